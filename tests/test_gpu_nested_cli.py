"""ipcr-nested end to end: `python -m ipcr_amd.nested_cli` against rows built from the oracle (outer products from the
record bytes, the best inner product from the exact amplicon bytes, internal/visitors/nested.go:35-51), its three data
paths (resident, resident --chunk-size, streamed chunks), ipcr_nested_products after ipcr_scan_genome_chunked and
ipcr_nested_scratch_products after ipcr_scan_chunk."""
import io
import json
import random

import pytest

import ipcr_oracle as O

pytestmark = pytest.mark.gpu

OUT_F = "ACGTTGCATGCAAGCTTAGC"
OUT_R = "GGCCTTAAGGCCATATCGTA"
IN1 = ("in1", "TTGACCGATTAC", "CCGGTTAACGGA")
IN2 = ("in2", "GATTACAGGTCA", "ACGGATTCAGGC")
INNER_TSV = [IN1, IN2, ("in2b",) + IN2[1:]]       # in2b == in2: identical products, the pair ID decides
OCFG = dict(max_mm=1, terminal_window=0, max_len=2000, hit_cap=10000, seed_len=12)
BASE_ARGS = ["-m", "1", "--terminal-window", "0"]


def rc(s: str) -> str:
    return O.revcomp(s).decode()


def acgt(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def plant_inner(s, b, pair, iln, mm_at=None):
    f = list(pair[1])
    if mm_at is not None:
        f[mm_at] = O.different_base(f[mm_at])
    s[b:b + 12] = f
    s[b + iln - 12:b + iln] = rc(pair[2])


def nested_record(rng, length=30_000):
    """outer amplicons of 300-1400 bp: without inner product, with one, with tying inner candidates; an N run, lower
    case and IUPAC bytes inside amplicons"""
    s = list(acgt(rng, length))
    lower = []
    for t in range(6):
        a = 1500 + t * ((length - 3000) // 6)
        ln = (300, 700, 1100, 1400, 500, 900)[t]
        s[a:a + 20] = OUT_F
        s[a + ln - 20:a + ln] = rc(OUT_R)
        if t % 3 == 1:
            plant_inner(s, a + 40, IN1, 150, mm_at=2 if t == 4 else None)
            if t == 4:
                s[a + 40 + 5] = "R"                       # an IUPAC byte inside the inner site: a hard mismatch
        elif t % 3 == 2:
            plant_inner(s, a + 30, IN2, 120)               # two equal candidates: the leftmost wins
            plant_inner(s, a + 200, IN2, 120)
            plant_inner(s, a + 60, IN1, 100, mm_at=3)      # shorter, with a mismatch: loses
            s[a + 25] = "Y"
        if t == 3:
            s[a + 200:a + 206] = "NNNNNN"
        if t == 1:
            lower.append((a, a + ln))
    out = "".join(s)
    for a, b in lower:
        out = out[:a] + out[a:b].lower() + out[b:]
    return out


def circular_record(rng, length=8000):
    """an outer product across the origin that holds an inner product across the origin"""
    s = list(acgt(rng, length))
    s[length - 150:length - 130] = OUT_F
    s[length - 100:length - 88] = IN1[1]
    s[40:52] = rc(IN1[2])
    s[120:140] = rc(OUT_R)
    s[length - 60] = "K"
    return "".join(s)


def write_fa(path, recs):
    with open(path, "w") as fh:
        for name, seq in recs:
            fh.write(f">{name} some description\n")
            for i in range(0, len(seq), 70):
                fh.write(seq[i:i + 70] + "\n")


def write_tsv(path, pairs):
    with open(path, "w") as fh:
        fh.write("# id fwd rev\n")
        for p in pairs:
            fh.write("\t".join(map(str, p)) + "\n")


def self_pairs(pairs):  # internal/common/primers.go:11-37
    out = list(pairs)
    for p in pairs:
        out.append(O.Pair(p.id + "+A:self", p.forward, p.forward))
        out.append(O.Pair(p.id + "+B:self", p.reverse, p.reverse))
    return out


def best_inner(amp: bytes, inner_pairs):
    hits = O.simulate_batch(O.Config(max_mm=1, terminal_window=0, seed_len=12), amp, inner_pairs)
    if not hits:
        return None
    return sorted(hits, key=lambda h: (h.fwd_mm + h.rev_mm, -h.length, h.start, h.end, h.experiment_id))[0]


def expected_rows(path, recs, outer_pairs, inner_pairs, circular=False):
    """(source_file, NestedProduct, seq) in the reference's emission order, from the oracle alone"""
    from ipcr_amd import engine, nested
    rows = []
    for name, seq in recs:
        b = seq.upper().encode()
        for p in O.simulate_batch(O.Config(circular=circular, **OCFG), b, outer_pairs):
            amp = b[p.start:p.end] if p.start <= p.end else b[p.start:] + b[:p.end]
            ep = engine.Product(p.experiment_id, name, p.start, p.end, p.length, p.type, p.fwd_mm, p.rev_mm,
                                tuple(p.fwd_idx), tuple(p.rev_idx))
            h = best_inner(amp, inner_pairs)
            np = nested.NestedProduct(ep, False) if h is None else nested.NestedProduct(
                ep, True, h.experiment_id, h.start, h.end, h.length, h.type, h.fwd_mm, h.rev_mm)
            rows.append((path, np, amp.decode("latin-1")))
    return rows


def render(rows, output, sort, require_inner, header=True):
    from ipcr_amd import nested_cli as N
    rows = [r for r in rows if r[1].InnerFound or not require_inner]
    if sort:
        rows = N.sort_rows(rows)
    if output == "json":
        return N.format_json(rows)
    if output == "jsonl":
        return "".join(N.format_jsonl(*r) + "\n" for r in rows)
    return (N.TSV_HEADER_NESTED + "\n" if header else "") + "".join(N.format_row(r[0], r[1]) + "\n" for r in rows)


def run_cli(args):
    from ipcr_amd import nested_cli
    out, err = io.StringIO(), io.StringIO()
    rc_ = nested_cli.run(args, stdout=out, stderr=err)
    assert rc_ == 0, err.getvalue()
    return out.getvalue()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("nested")
    rng = random.Random(2024)
    recs = [("chrA", nested_record(rng)), ("chrB", nested_record(rng, 26_000)), ("plasmid", nested_record(rng, 22_000))]
    fa = d / "g.fa"
    write_fa(fa, recs)
    write_tsv(d / "outer.tsv", [("O1", OUT_F, OUT_R, 0, 2000)])
    write_tsv(d / "inner.tsv", INNER_TSV)
    return d, recs


@pytest.mark.parametrize("inner_src", ["inline", "tsv"])
@pytest.mark.parametrize("self_", [True, False])
def test_cli_matches_oracle(files, inner_src, self_):
    d, recs = files
    fa = str(d / "g.fa")
    if inner_src == "inline":
        outer_args, inner_args = ["-f", OUT_F, "-r", OUT_R], ["-F", IN1[1], "-R", IN1[2]]
        outer = [O.Pair("outer", OUT_F, OUT_R, 0, 2000)]
        inner = [O.Pair("inner", IN1[1], IN1[2])]
    else:
        outer_args, inner_args = ["--outer-primers", str(d / "outer.tsv")], ["--inner-primers", str(d / "inner.tsv")]
        outer = [O.Pair("O1", OUT_F, OUT_R, 0, 2000)]
        inner = [O.Pair(*p) for p in INNER_TSV]
    if self_:
        outer, inner = self_pairs(outer), self_pairs(inner)
    rows = expected_rows(fa, recs, outer, inner)
    n_found = sum(r[1].InnerFound for r in rows)
    assert len(rows) >= 18 and 0 < n_found < len(rows)
    if inner_src == "tsv":   # the tie between in2 and in2b went to in2, and the leftmost equal candidate won
        assert any(r[1].InnerPairID == "in2" and r[1].InnerStart == 30 for r in rows)
    assert any(set(r[2]) - set("ACGT") for r in rows), "no byte outside ACGT inside an amplicon"
    flags = BASE_ARGS + outer_args + inner_args + ([] if self_ else ["--no-self"])
    for output in ("text", "jsonl", "json"):
        for sort in (False, True):
            for req in (False, True):
                args = flags + ["-o", output] + (["--sort"] if sort else []) + (["--require-inner"] if req else []) + [fa]
                assert run_cli(args) == render(rows, output, sort, req), (output, sort, req)


@pytest.mark.parametrize("output", ["text", "jsonl"])
def test_chunked_equals_unchunked(files, monkeypatch, output):
    d, recs = files
    fa = str(d / "g.fa")
    args = BASE_ARGS + ["--outer-primers", str(d / "outer.tsv"), "--inner-primers", str(d / "inner.tsv"), "-o", output]
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    whole = run_cli(args + [fa])
    whole_sorted = run_cli(args + ["--sort", fa])
    assert len(whole.splitlines()) >= 18
    for stream in ("", "1"):
        monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", stream)
        chunked = run_cli(args + ["--chunk-size", "4000", "--sort", fa])
        assert chunked == whole_sorted, stream
        assert sorted(run_cli(args + ["--chunk-size", "4000", fa]).splitlines()) == sorted(whole.splitlines()), stream
        req = run_cli(args + ["--chunk-size", "4000", "--sort", "--require-inner", fa])
        assert req == run_cli(args + ["--sort", "--require-inner", fa]), stream


def test_circular_product_across_the_origin(tmp_path, monkeypatch):
    rng = random.Random(77)
    recs = [("circ", circular_record(rng)), ("lin", nested_record(rng, 12_000))]
    fa = str(tmp_path / "c.fa")
    write_fa(tmp_path / "c.fa", recs)
    outer = self_pairs([O.Pair("outer", OUT_F, OUT_R, 0, 2000)])
    inner = self_pairs([O.Pair("inner", IN1[1], IN1[2])])
    rows = expected_rows(fa, recs, outer, inner, circular=True)
    wrap = [r for r in rows if r[1].Product.Start > r[1].Product.End]
    assert wrap and wrap[0][1].InnerFound
    args = BASE_ARGS + ["-f", OUT_F, "-r", OUT_R, "-F", IN1[1], "-R", IN1[2], "--circular"]
    for output in ("text", "jsonl", "json"):
        assert run_cli(args + ["-o", output, fa]) == render(rows, output, False, False), output
    # chunking is disabled for circular templates (runutil.go:46-49): the same output, with a warning
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "1")
    assert run_cli(args + ["-o", "jsonl", "--chunk-size", "3000", fa]) == render(rows, "jsonl", False, False)


def test_no_match_exit_code(files):
    from ipcr_amd import nested_cli
    d, _ = files
    out, err = io.StringIO(), io.StringIO()
    args = BASE_ARGS + ["-f", OUT_F, "-r", OUT_R, "-F", "ACACACACACAC", "-R", "GTGTGTGTGTGT", "--no-self",
                        "--require-inner", "--no-match-exit-code", "7", str(d / "g.fa")]
    assert nested_cli.run(args, stdout=out, stderr=err) == 7
    assert out.getvalue() == nested_cli.TSV_HEADER_NESTED + "\n"


def _key(np):
    return (np.InnerFound, np.InnerPairID, np.InnerStart, np.InnerEnd, np.InnerLength, np.InnerType, np.InnerFwdMM,
            np.InnerRevMM)


def _panels(circular=False):
    from ipcr_amd import engine, primer
    oeng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, MaxLen=2000, HitCap=10000, SeedLen=12, Circular=circular))
    cpo = oeng.CompilePanel(primer.AddSelfPairs([primer.Pair("O1", OUT_F, OUT_R, 0, 2000)]))
    ieng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, SeedLen=12))
    cpi = ieng.CompilePanel(primer.AddSelfPairs([primer.Pair(*p) for p in INNER_TSV]))
    return oeng, cpo, ieng, cpi


def test_nested_products_after_chunked_scan(files):
    """window-local products of ipcr_scan_genome_chunked are put back into their records before the gather"""
    from ipcr_amd import engine, nested
    _, recs = files
    g = engine.Genome(1 << 20, 8)
    for name, seq in recs:
        g.add_record(name, seq.upper().encode())
    oeng, cpo, ieng, cpi = _panels()
    sco, scc, sci = oeng.NewSimulationScratch(cpo), oeng.NewSimulationScratch(cpo), ieng.NewSimulationScratch(cpi)
    whole = oeng.ScanGenome(g, cpo, sco)
    want = {(p.Record, p.Start, p.End, p.ExperimentID, p.Type): _key(n)
            for p, n in zip(whole, nested.NestedProducts(sco, whole, g, cpi, sci))}
    chunked = oeng.ScanGenomeChunked(g, cpo, scc, 4000, 2000)
    got = nested.NestedProducts(scc, chunked, g, cpi, sci)
    w = scc.chunk_windows()
    assert len(chunked) > len(whole) >= 18       # products in the overlap of two windows come twice
    found = 0
    for p, n in zip(chunked, got):
        cw = w[p.Record]
        k = (cw.record, cw.start + p.Start, cw.start + p.End, p.ExperimentID, p.Type)
        assert k in want, k
        assert _key(n) == want[k], (k, _key(n), want[k])
        found += n.InnerFound
    assert found >= 6
    g.close()


def test_nested_scratch_products_vs_windows(files):
    """the products of an ipcr_scan_chunk, their amplicons read from the chunk's own tiles == NestedWindows over the same
    amplicons of a resident genome; a circular chunk's wrap-around product included"""
    from ipcr_amd import engine, nested
    _, recs = files
    rng = random.Random(5)
    circ = circular_record(rng)
    all_recs = [s.upper() for _, s in recs] + [circ]
    g = engine.Genome(1 << 20, 8)
    for r, s in enumerate(all_recs):
        g.add_record("r%d" % r, s.encode())
    found = 0
    for circular in (False, True):
        oeng, cpo, ieng, cpi = _panels(circular)
        sco, sci, sci2 = oeng.NewSimulationScratch(cpo), ieng.NewSimulationScratch(cpi), ieng.NewSimulationScratch(cpi)
        chunks = [(len(all_recs) - 1, 0, len(circ))] if circular else \
            [(r, a, min(a + 9000, len(all_recs[r]))) for r in range(len(recs)) for a in range(0, len(all_recs[r]), 7000)]
        wraps = 0
        for r, a, b in chunks:
            prods = oeng.SimulateCompiledWithScratch("c", all_recs[r][a:b].encode(), cpo, sco)
            got = nested.NestedScratchProducts(sco, prods, cpi, sci)
            assert len(got) == len(prods)
            if not prods:
                continue
            want = nested.NestedWindows(g, [(r, a + p.Start, a + p.End) if p.Start <= p.End else (r, p.Start, p.End)
                                            for p in prods], cpi, sci2)
            assert [_key(n) for n in got] == [_key(n) for n in want]
            assert [n.Product for n in got] == prods
            found += sum(n.InnerFound for n in got)
            wraps += sum(p.Start > p.End for p in prods)
        if circular:
            assert wraps >= 1
    assert found >= 6
    assert len(nested.NestedScratchProducts(sco, prods, cpi, sci, require_inner=True)) == sum(n.InnerFound for n in got)
    g.close()


def test_nested_scratch_products_errors_and_empty():
    from ipcr_amd import _lib, engine, nested
    oeng, cpo, ieng, cpi = _panels()
    sco, sci = oeng.NewSimulationScratch(cpo), ieng.NewSimulationScratch(cpi)
    L = _lib.lib()
    out = (_lib.NestedHit * 4)()

    def status(outer, inner_sc, n):
        return L.ipcr_nested_scratch_products(outer._h, cpi._h, inner_sc._h, out, n)

    assert status(sco, sci, 0) == _lib.ERR_INVALID                     # never scanned
    seq = "A" * 3000 + OUT_F + acgt(random.Random(1), 400) + rc(OUT_R) + "C" * 2000
    prods = oeng.SimulateCompiledWithScratch("x", seq.encode(), cpo, sco)
    assert len(prods) == 1
    assert status(sco, sco, 1) == _lib.ERR_INVALID                     # outer == inner scratch
    assert status(sco, sci, 2) == _lib.ERR_INVALID                     # n_out != products
    host = engine.SimulationScratch(cpi, host_only=True)
    assert status(sco, host, 1) == _lib.ERR_DEVICE                     # a host-only scratch cannot scan
    assert len(nested.NestedScratchProducts(sco, prods, cpi, sci)) == 1
    # an empty chunk scan: OK, nothing written
    assert oeng.SimulateCompiledWithScratch("y", b"ACGT" * 1000, cpo, sco) == []
    out[0].found = 77
    assert status(sco, sci, 0) == _lib.OK and out[0].found == 77
    assert nested.NestedScratchProducts(sco, [], cpi, sci) == []
    # the last scan on the outer scratch was over a resident genome, not a chunk
    g = engine.Genome(1 << 16, 2)
    g.add_record("r", seq.encode())
    assert len(oeng.ScanGenome(g, cpo, sco)) == 1
    assert status(sco, sci, 1) == _lib.ERR_INVALID
    with pytest.raises(_lib.IpcrError):
        nested.NestedScratchProducts(sco, [None], cpi, sci)
    g.close()
    host.close()


def _nested_args(d):
    return BASE_ARGS + ["--outer-primers", str(d / "outer.tsv"), "--inner-primers", str(d / "inner.tsv")]


@pytest.mark.parametrize("mode", ["whole", "chunk", "chunk_stream"])
def test_unreadable_file_between_two_good_ones(files, tmp_path, monkeypatch, mode):
    """pipeline.go:174-182: a file that cannot be read is reported and the next one is scanned"""
    from ipcr_amd import nested_cli
    d, recs = files
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "1" if mode == "chunk_stream" else "")
    a, b = str(d / "g.fa"), str(tmp_path / "b.fa")
    write_fa(b, recs[1:])
    args = _nested_args(d) + (["--chunk-size", "4000"] if mode != "whole" else [])
    only_a, only_b = run_cli(args + [a]), run_cli(args + [b])
    assert len(only_a.splitlines()) >= 19 and len(only_b.splitlines()) >= 7
    out, err = io.StringIO(), io.StringIO()
    assert nested_cli.run(args + [a, str(tmp_path / "missing.fa"), b], stdout=out, stderr=err) == 0
    assert out.getvalue().splitlines() == only_a.splitlines() + only_b.splitlines()[1:]
    assert [ln[:6] for ln in err.getvalue().splitlines()] == ["error:"], err.getvalue()


def test_chunked_scan_falls_back_to_streamed_chunks_after_a_segmented_capped_scan(tmp_path, monkeypatch):
    """as the test of this name in test_gpu_fasta.py: ipcr_scan_genome_chunked refuses after a capped scan that ran in
    segments, the driver streams the chunks -- the output of IPCR_CLI_STREAM_CHUNKS=1"""
    from ipcr_amd import _lib, engine, primer
    monkeypatch.setenv("IPCR_TEST_HCAP_SOFT", "30000")
    rng = random.Random(9)
    fa = tmp_path / "polya.fa"
    recs = []
    for r in range(3):
        s = bytearray(b"A" * 400_000)
        for _ in range(40):
            s[rng.randrange(len(s))] = rng.choice(b"CGTNn")
        recs.append(("r%d" % r, s.decode()))
    write_fa(fa, recs)
    fwd, rev = "AAAAAAAAAAAA", "TTTTTTTTTTTT"
    eng = engine.New(engine.Config(MaxMM=0, TerminalWindow=3, MaxLen=60, HitCap=50, SeedLen=12))
    cp = eng.CompilePanel(primer.AddSelfPairs([primer.Pair("outer", fwd, rev, 0, 60)]))
    sc = eng.NewSimulationScratch(cp)
    g = engine.Genome(1 << 22, 4)
    g.add_fasta(str(fa))
    with pytest.raises(_lib.IpcrError) as e:                             # the branch under test is reached
        eng.ScanGenomeChunked(g, cp, sc, 100_000, 60)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    g.close(); sc.close(); cp.close()
    base = ["-f", fwd, "-r", rev, "-F", "AAAAAAAA", "-R", "TTTTTTTT", "--hit-cap", "50", "--max-length", "60",
            "--chunk-size", "100000", "-o", "jsonl", str(fa)]
    for extra in ([], ["--sort"]):
        monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
        got = run_cli(base + extra)
        monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "1")
        assert got == run_cli(base + extra) and len(got.splitlines()) > 100, extra
    assert any(json.loads(ln)["inner_found"] for ln in got.splitlines())


def test_sequences_from_a_genome_without_exception_runs(tmp_path, monkeypatch):
    """a genome that kept no exception runs (IPCR_TEST_EXCEPTION_MAX lowers the bound): ipcr_genome_read_windows refuses and
    `seq` comes from the file instead -- the same JSONL as with the runs kept, whole records and --chunk-size"""
    from ipcr_amd import _lib, engine
    rng = random.Random(31)
    s = list(nested_record(rng))
    for p in range(26_000, 30_000, 20):                                  # > 100 runs, behind the last amplicon
        s[p] = "R"
    fa = tmp_path / "g.fa"
    write_fa(fa, [("chrA", "".join(s))])
    write_tsv(tmp_path / "outer.tsv", [("O1", OUT_F, OUT_R, 0, 2000)])
    write_tsv(tmp_path / "inner.tsv", INNER_TSV)
    base = _nested_args(tmp_path) + ["-o", "jsonl", str(fa)]
    forms = [[], ["--chunk-size", "4000"]]
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    want = [run_cli(base + f) for f in forms]
    assert all(len(w.splitlines()) >= 6 for w in want)
    assert any(set(json.loads(ln)["seq"]) - set("ACGTN") for ln in want[0].splitlines())
    monkeypatch.setenv("IPCR_TEST_EXCEPTION_MAX", "100")
    g = engine.Genome(1 << 20, 4)
    g.add_fasta(str(fa))
    with pytest.raises(_lib.IpcrError) as e:                             # the branch under test is reached
        g.read_windows([(0, 0, 10)])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    g.close()
    for f, w in zip(forms, want):
        assert run_cli(base + f) == w, f
