"""Product sequences from resident genomes: read_windows over the products of ipcr_scan_genome (a wrap-around product of a
circular panel included) and ipcr_scan_genome_chunked (window-local coordinates mapped back), and the CLI's --output fasta
and --products, with IUPAC codes and gaps planted inside the amplicons."""
import gzip
import io
import json
import random

import pytest

pytestmark = pytest.mark.gpu

FW = "AGAGTTTGATCMTGGCTCAG"      # 27F-style (IUPAC M)
RV = "TACGGYTACCTTGTTAYGACTT"    # 1492R-style (IUPAC Y)


def acgt(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def site(p, rng):
    """a concrete site for an IUPAC primer"""
    pick = {"M": "AC", "Y": "CT", "R": "AG", "K": "GT", "S": "CG", "W": "AT"}
    return "".join(rng.choice(pick[c]) if c in pick else c for c in p).encode()


def revcomp(b):
    return b.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def amplicon_record(rng, n_amp=4, length=40_000, wrap=False):
    """ACGT with products [fw site ... rc(rv) site], IUPAC codes and gaps planted between the sites"""
    s = bytearray(acgt(rng, length))
    for k in range(n_amp):
        a = 2000 + k * 8000
        amp = bytearray(site(FW, rng) + acgt(rng, 300 + 37 * k) + revcomp(site(RV, rng)))
        for j in range(25, len(amp) - 25, 23):
            amp[j] = rng.choice(b"RYKMSWBDHVN-")
        amp[40:44] = b"----"
        s[a:a + len(amp)] = amp
    if wrap:  # a product across the origin: the forward site near the end, the reverse site at the start
        f = site(FW, rng)
        s[length - 120:length - 120 + len(f)] = f
        s[length - 60] = ord("R")
        r = revcomp(site(RV, rng))
        s[80:80 + len(r)] = r
        s[30] = ord("Y")
    return bytes(s)


def engine_for(circular=False, chunk=False):
    from ipcr_amd import engine, primer
    cfg = engine.Config(MaxMM=3, TerminalWindow=0, MinLen=50, MaxLen=2000, HitCap=0, SeedLen=12, Circular=circular)
    eng = engine.New(cfg)
    pairs = [primer.Pair("C3", primer.Validate(FW), primer.Validate(RV), 50, 2000)]
    pairs = primer.AddSelfPairs(pairs)
    cp = eng.CompilePanel(pairs)
    return eng, cp, eng.NewSimulationScratch(cp)


def slice_of(rec, s, e):
    return rec[s:e] if s <= e else rec[s:] + rec[:e]


def test_scan_genome_products_exact():
    from ipcr_amd import engine
    rng = random.Random(1)
    recs = [amplicon_record(rng, wrap=True), amplicon_record(rng, 3, 30_000)]
    g = engine.Genome(200_000, 4)
    for i, r in enumerate(recs):
        g.add_record("r%d" % i, r)
    eng, cp, sc = engine_for(circular=True)
    prods = eng.ScanGenome(g, cp, sc)
    assert len(prods) >= 7
    assert any(p.Start > p.End for p in prods), "no wrap-around product"
    got = g.read_windows([(p.Record, p.Start, p.End) for p in prods])
    for p, b in zip(prods, got):
        assert b == slice_of(recs[p.Record], p.Start, p.End), (p.Record, p.Start, p.End)
    assert any(set(b) - set(b"ACGTN") for b in got)
    g.close()


def test_scan_genome_chunked_products_exact():
    from ipcr_amd import engine
    rng = random.Random(2)
    recs = [amplicon_record(rng, 4, 40_000), amplicon_record(rng, 2, 20_000)]
    g = engine.Genome(200_000, 4)
    for i, r in enumerate(recs):
        g.add_record("r%d" % i, r)
    eng, cp, sc = engine_for()
    prods = eng.ScanGenomeChunked(g, cp, sc, 3000, 2000)
    w = sc.chunk_windows()
    win = [(w[p.Record].record, w[p.Record].start + p.Start, w[p.Record].start + p.End) for p in prods]
    assert len(win) >= 6
    got = g.read_windows(win)
    for (r, s, e), b in zip(win, got):
        assert b == recs[r][s:e]
    g.close()


# ---- the CLI ------------------------------------------------------------------------------------------------------------

def cli(args):
    from ipcr_amd import cli as C
    out, err = io.StringIO(), io.StringIO()
    rc = C.run(args, stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    return out.getvalue()


def write_fa(path, recs, gz=False):
    lines = []
    for i, r in enumerate(recs):
        lines.append(b">rec%d some text" % i)
        for k, j in enumerate(range(0, len(r), 70)):
            piece = r[j:j + 70]
            lines.append(piece.lower() if k % 3 == 1 else piece)   # lower-case lines: normalised to upper case
    data = b"\n".join(lines) + b"\n"
    if gz:
        with gzip.open(path, "wb") as fh:
            fh.write(data)
    else:
        path.write_bytes(data)


def expected_fasta(text_out, recs, sort):
    """output/fasta.go restated over the text rows (the scan itself is pinned by the parity suites)"""
    rows = [ln.split("\t") for ln in text_out.splitlines()[1:]]
    out, written = [], 0
    for i, f in enumerate(rows):
        src, sid, exp, s, e, ln = f[0], f[1], f[2], int(f[3]), int(f[4]), int(f[5])
        seq = slice_of(recs[int(sid[3:])], s, e).decode()
        if not seq:
            continue
        written += 1
        out.append(">%s_%d start=%d end=%d len=%d source_file=%s\n%s\n" % (exp, i + 1 if sort else written, s, e, ln, src, seq))
    return "".join(out)


@pytest.mark.parametrize("case", ["plain", "sort", "chunk", "chunk_stream", "gzip", "circular"])
def test_cli_fasta_output(tmp_path, monkeypatch, case):
    rng = random.Random(10)
    recs = [amplicon_record(rng, 4, 40_000, wrap=case == "circular"), amplicon_record(rng, 2, 20_000)]
    fa = tmp_path / ("g.fa.gz" if case == "gzip" else "g.fa")
    write_fa(fa, recs, gz=case == "gzip")
    args = ["-f", FW, "-r", RV, "-m", "3", "--terminal-window", "0", "--min-length", "50", str(fa)]
    if case in ("chunk", "chunk_stream"):
        args += ["--chunk-size", "3000"]
        monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "1" if case == "chunk_stream" else "")
    if case == "circular":
        args += ["--circular"]
    if case == "sort":
        args += ["--sort"]
    text = cli(args)
    assert len(text.splitlines()) > 4
    if case == "circular":
        assert any(int(f.split("\t")[3]) > int(f.split("\t")[4]) for f in text.splitlines()[1:])
    got = cli(args + ["--output", "fasta"])
    assert got == expected_fasta(text, recs, case == "sort")
    assert set("".join(got.splitlines()[1::2])) - set("ACGTN"), "no byte outside ACGTN inside the products"


def test_cli_products_jsonl_and_text(tmp_path):
    rng = random.Random(11)
    recs = [amplicon_record(rng, 4, 40_000)]
    fa = tmp_path / "g.fa"
    write_fa(fa, recs)
    args = ["-f", FW, "-r", RV, "-m", "3", "--terminal-window", "0", "--min-length", "50", str(fa)]
    plain = cli(args + ["-o", "jsonl"]).splitlines()
    withseq = cli(args + ["-o", "jsonl", "--products"]).splitlines()
    assert len(plain) == len(withseq) > 2
    for a, b in zip(plain, withseq):
        da, db = json.loads(a), json.loads(b)
        seq = db.pop("seq")
        assert da == db
        assert seq.encode() == recs[0][da["start"]:da["end"]]
        assert list(json.loads(b).keys())[-2:] == ["seq", "source_file"]
    assert cli(args) == cli(args + ["--products"])


def test_cli_sequences_from_a_genome_without_exception_runs(tmp_path, monkeypatch):
    """A genome with more runs of bytes outside ACGTacgtN than its bound keeps none (IPCR_TEST_EXCEPTION_MAX lowers the bound)
    and ipcr_genome_read_windows refuses: the driver takes the amplicon bytes from the file instead -- the same output as
    with the runs kept, whole records and --chunk-size."""
    from ipcr_amd import _lib, engine
    rng = random.Random(12)
    recs = []
    for n_amp, length in ((4, 40_000), (2, 20_000)):
        s = bytearray(amplicon_record(rng, n_amp, length))
        for p in range(length * 3 // 4, length, 50):                     # > 100 runs, behind the last amplicon
            s[p] = ord("R")
        recs.append(bytes(s))
    fa = tmp_path / "g.fa"
    write_fa(fa, recs)
    base = ["-f", FW, "-r", RV, "-m", "3", "--terminal-window", "0", "--min-length", "50", str(fa)]
    forms = [out + chunk for out in (["-o", "jsonl", "--products"], ["-o", "fasta"]) for chunk in ([], ["--chunk-size", "3000"])]
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    want = [cli(base + f) for f in forms]
    assert all(len(w.splitlines()) >= 6 for w in want)
    assert set("".join(want[2].splitlines()[1::2])) - set("ACGTN"), "no byte outside ACGTN inside the products"
    monkeypatch.setenv("IPCR_TEST_EXCEPTION_MAX", "100")
    g = engine.Genome(1 << 20, 4)
    g.add_fasta(str(fa))
    with pytest.raises(_lib.IpcrError) as e:                             # the branch under test is reached
        g.read_windows([(0, 0, 10)])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    g.close()
    for f, w in zip(forms, want):
        assert cli(base + f) == w, f
