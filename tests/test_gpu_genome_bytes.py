"""Exact bytes from resident genomes: the exception runs every tile writer keeps (bytes outside ACGTacgtN, which the tiles
decode as 'N') and ipcr_genome_read_windows, which puts them back.  Every writer path must round-trip the loaded bytes
exactly, for windows of every shape; exception_runs must equal the count of maximal same-byte runs."""
import ctypes
import gzip
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

COL = 4096
UINT64_MAX = (1 << 64) - 1
EDGES = (127, 128, 4095, 4096, 8191, 8192, 262143, 262144)


def record_cols(n):
    return (n + 128 + 8191) // 8192 * 2


def acgt(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def runs_of(seqs):
    """maximal runs of one byte value outside ACGTacgtN, over every record"""
    n = 0
    for s in seqs:
        prev = None
        for b in s:
            if b not in b"ACGTacgtN" and b != prev:
                n += 1
            prev = b
    return n


def planted(rng, n, extra=b"", lower=False):
    """n bases with IUPAC codes, U, gaps, digits and `extra` planted at record, column, pair and block edges, neighbours
    of different codes, one run across a pack-pair edge, and N runs"""
    s = bytearray(acgt(rng, n))
    if lower:
        for i in range(0, n, 7):
            s[i] = s[i] | 0x20
    codes = b"RYKMSWBDHVU-.*X0123456789" + extra
    for k, p in enumerate(e for e in EDGES if e < n):
        s[p] = codes[k % len(codes)]
    for p in (0, n - 1):
        s[p] = codes[(p * 7) % len(codes)]
    for p in range(150, min(n, 40_000), 997):
        s[p] = codes[(p // 997) % len(codes)]
    if n > 9000:
        s[8180:8200] = b"R" * 20             # one run across the pack-pair edge 8192
        s[6000:6004] = b"RRYY"
        s[7000:7100] = b"N" * 100             # N adds no run
    return bytes(s)


def windows_for(seqs, rng):
    win = []
    for r, s in enumerate(seqs):
        n = len(s)
        for ln in (0, 1, 31, 32, 127, 128, 4096, 100_000):
            if ln <= n:
                for st in {0, n - ln, min(n - ln, 8190), rng.randrange(n - ln + 1)}:
                    win.append((r, st, st + ln))
        for e in EDGES:
            if e + 3 <= n:
                win.append((r, e - 2 if e >= 2 else 0, e + 3))
        if n > 10:
            win.append((r, n - 5, 7))           # across the origin
            win.append((r, n, 0))
    return win


def want_of(seqs, win):
    out = []
    for r, s, e in win:
        b = seqs[r]
        out.append(b[s:e] if s <= e else b[s:] + b[:e])
    return out


def check(g, seqs, what):
    rng = random.Random(len(seqs))
    win = windows_for(seqs, rng)
    got = g.read_windows(win)
    bad = [(w, got[i][:40], want_of(seqs, [w])[0][:40]) for i, w in enumerate(win) if got[i] != want_of(seqs, [w])[0]]
    assert not bad, (what, len(bad), bad[:3])
    assert g.exception_runs == runs_of(seqs), (what, g.exception_runs, runs_of(seqs))
    assert g.read_windows([]) == []


def new_genome(seqs, extra_records=2):
    from ipcr_amd import engine
    return engine.Genome(sum(record_cols(len(s)) for s in seqs) * COL + 4 * 8192, len(seqs) + extra_records)


def test_add_record_short():
    seqs = [planted(random.Random(i), n, b"n r\t\x80\xff", lower=True) for i, n in enumerate((1, 31, 200, 4095))]
    g = new_genome(seqs)
    for i, s in enumerate(seqs):
        g.add_record("r%d" % i, s)
    check(g, seqs, "add_record < 4096")
    g.close()


@pytest.mark.parametrize("bar", ["1", "0"])
def test_add_record_long(monkeypatch, bar):
    from ipcr_amd import _lib
    monkeypatch.setenv("IPCR_CHUNK_BAR", bar)
    if bar == "1":
        f = getattr(_lib.lib(), "ipcr_internal_bar_writable", None)
        if f is not None:
            f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int]
            if not f(0):
                pytest.skip("the host has no large BAR on device 0: the host-packed path is not taken")
    seqs = [planted(random.Random(10 + i), n, b"nr\x80", lower=True) for i, n in enumerate((4096, 300_000, 600_000))]
    g = new_genome(seqs)
    for i, s in enumerate(seqs):
        g.add_record("r%d" % i, s)
    check(g, seqs, "add_record BAR=" + bar)
    g.close()


def test_add_record_device():
    import torch
    seqs = [planted(random.Random(20 + i), n, b"n\x90", lower=True) for i, n in enumerate((100, 5000, 270_000))]
    g = new_genome(seqs)
    for i, s in enumerate(seqs):
        buf = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        g.add_record_device("r%d" % i, buf.data_ptr(), len(s))
        del buf
    check(g, seqs, "add_record_device")
    g.close()


def write_fasta(path, seqs, width=60, ragged=False, gz=False, lower=False):
    lines = []
    rng = random.Random(5)
    for i, s in enumerate(seqs):
        lines.append(b">r%d desc" % i)
        j = 0
        while j < len(s):
            w = rng.randrange(20, 90) if ragged else width
            piece = s[j:j + w]
            lines.append(piece.lower() if lower and (j // w) % 2 else piece)
            j += w
    data = b"\n".join(lines) + b"\n"
    if gz:
        with gzip.open(path, "wb") as fh:
            fh.write(data)
    else:
        with open(path, "wb") as fh:
            fh.write(data)


def fasta_records(n, seed, inner_blank=False):
    """normalised FASTA text: upper case (normalize.go), no blanks at line ends"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        s = bytearray(planted(rng, rng.choice((300, 9000, 70_000)) if n > 4 else 300_000))
        if inner_blank and len(s) > 50:
            s[40] = ord(" ")
            s[45] = ord("\t")
        out.append(bytes(s))
    return out


@pytest.mark.parametrize("case", ["hostpack", "device", "gzip", "ragged", "slab64", "many", "blank"])
def test_add_fasta(tmp_path, monkeypatch, case):
    nrec = 300 if case == "many" else 6 if case == "slab64" else 4
    seqs = fasta_records(nrec, 30 + nrec, inner_blank=case == "blank")
    path = tmp_path / ("g.fa.gz" if case == "gzip" else "g.fa")
    if case == "blank":  # a blank inside a line is kept (TrimSpace trims line ends only): lay the lines out around it
        with open(path, "wb") as fh:
            for i, s in enumerate(seqs):
                fh.write(b">r%d\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n")
    else:
        write_fasta(path, seqs, ragged=case == "ragged", gz=case == "gzip", lower=case in ("device", "ragged"))
    if case != "hostpack":
        monkeypatch.setenv("IPCR_FASTA_HOSTPACK", "0")
    if case == "slab64":
        monkeypatch.setenv("IPCR_FASTA_SLAB", "64")
    g = new_genome(seqs)
    assert g.add_fasta(str(path)) == nrec
    check(g, seqs, "fasta " + case)
    g.close()


def test_acgtn_genome_keeps_no_runs():
    rng = random.Random(40)
    s = bytearray(acgt(rng, 300_000))
    s[1000:2000] = b"N" * 1000
    s[5000:5100] = bytes(acgt(rng, 100)).lower()
    g = new_genome([bytes(s)])
    g.add_record("r", bytes(s))
    assert g.exception_runs == 0
    assert g.read_windows([(0, 900, 2100)]) == [bytes(s[900:2100])]
    g.close()


def test_overflow_redo(monkeypatch, tmp_path):
    monkeypatch.setenv("IPCR_TEST_EXCEPTION_CAP", "1")
    seqs = [planted(random.Random(50 + i), n) for i, n in enumerate((300, 20_000, 300_000))]
    g = new_genome(seqs)
    for i, s in enumerate(seqs):
        g.add_record("r%d" % i, s)
    check(g, seqs, "add_record, capacity 1")
    g.close()
    monkeypatch.setenv("IPCR_FASTA_HOSTPACK", "0")
    monkeypatch.setenv("IPCR_FASTA_SLAB", "64")
    seqs = fasta_records(8, 51)
    write_fasta(tmp_path / "g.fa", seqs)
    g = new_genome(seqs)
    assert g.add_fasta(str(tmp_path / "g.fa")) == 8
    check(g, seqs, "fasta, capacity 1")
    g.close()


def scan_products(g, seq):
    from ipcr_amd import engine, primer
    rc = primer.RevComp(seq[3000:3021].decode())
    fw, rv = seq[1000:1020].decode(), rc.decode() if isinstance(rc, (bytes, bytearray)) else rc
    eng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, MinLen=10, MaxLen=5000, HitCap=0, SeedLen=12))
    cp = eng.CompilePanel([primer.Pair("p", fw, rv, 10, 5000)])
    sc = eng.NewSimulationScratch(cp)
    return [(p.sig(), p.Record) for p in eng.ScanGenome(g, cp, sc)]


def test_bound_drops_runs(monkeypatch):
    from ipcr_amd import _lib
    rng = random.Random(60)
    s = bytearray(acgt(rng, 300_000))
    for p in range(5000, 300_000, 50):
        s[p] = ord("R")
    s = bytes(s)
    g0 = new_genome([s])
    g0.add_record("r", s)
    want = scan_products(g0, s)
    assert g0.exception_runs == runs_of([s])
    g0.close()
    monkeypatch.setenv("IPCR_TEST_EXCEPTION_MAX", "100")
    g = new_genome([s])
    g.add_record("r", s)
    assert scan_products(g, s) == want
    assert g.exception_runs == UINT64_MAX
    with pytest.raises(_lib.IpcrError) as e:
        g.read_windows([(0, 0, 10)])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    g.close()


def test_errors():
    from ipcr_amd import _lib
    s = planted(random.Random(70), 5000)
    g = new_genome([s])
    g.add_record("r", s)
    lib = _lib.lib()
    win = (_lib.Window * 2)()
    win[0].record, win[0].start, win[0].end = 0, 10, 110
    win[1].record, win[1].start, win[1].end = 0, 4990, 20
    offs = (ctypes.c_uint64 * 3)()
    need = ctypes.c_uint64()
    buf = ctypes.create_string_buffer(200)
    assert lib.ipcr_genome_read_windows(g._h, win, 2, buf, 50, offs, ctypes.byref(need)) == _lib.ERR_CAPACITY
    assert need.value == 130 and list(offs) == [0, 100, 130]
    assert lib.ipcr_genome_read_windows(g._h, win, 2, buf, 200, offs, ctypes.byref(need)) == _lib.OK
    assert buf.raw[:130] == s[10:110] + s[4990:] + s[:20]
    for bad in ((0, 0, 5001), (1, 0, 1), (0, -1, 3), (0, 5001, 0)):
        win[0].record, win[0].start, win[0].end = bad
        assert lib.ipcr_genome_read_windows(g._h, win, 1, buf, 200, offs, ctypes.byref(need)) == _lib.ERR_INVALID, bad
    g.close()


def test_concurrent_reads_next_to_a_scan():
    from ipcr_amd import engine, primer
    seqs = [planted(random.Random(80 + i), 300_000) for i in range(2)]
    g = new_genome(seqs)
    for i, s in enumerate(seqs):
        g.add_record("r%d" % i, s)
    rng = random.Random(81)
    win = [(rng.randrange(2), a, a + rng.randrange(1000, 2000)) for a in (rng.randrange(290_000) for _ in range(3000))]
    want = want_of(seqs, win)
    other = new_genome(seqs)
    other.add_record("x", seqs[0])
    eng = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=10, MaxLen=3000, HitCap=0, SeedLen=12))
    cp = eng.CompilePanel([primer.Pair("p", "ACGTACGTACGTACGTAC", "TTGCATTGCATTGCATTG", 10, 3000)])
    sc = eng.NewSimulationScratch(cp)
    results, errs = [None] * 4, []

    def reader(k):
        try:
            for _ in range(3):
                got = g.read_windows(win)
                if got != want:
                    results[k] = False
                    return
            results[k] = True
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    ts = [threading.Thread(target=reader, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for _ in range(3):
        eng.ScanGenome(other, cp, sc)
    for t in ts:
        t.join()
    assert not errs and results == [True] * 4
    g.close()
    other.close()
