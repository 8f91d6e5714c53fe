"""--pretty end to end: the CLI's alignment blocks against the reference's recorded output (tests/golden/pretty), and
`ipcr`, `ipcr --probe` and `ipcr-nested` against rows of the existing formatters interleaved with ipcr_amd.pretty's
rendering of sites this file sliced from the records it wrote (products from the oracle)."""
import io
import os
import random

import pytest

import ipcr_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretty")
COMP = {a: b for a, b in zip("ACGTRYSWKMBVDHN", "TGCAYRSWMKVBHDN")}


def rc(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def golden(name: str) -> str:
    with open(os.path.join(GOLDEN, name + ".golden"), "rb") as fh:
        return fh.read().decode("utf-8")


def run(mod, args):
    out, err = io.StringIO(), io.StringIO()
    code = mod.run(args, stdout=out, stderr=err)
    assert code == 0, err.getvalue()
    return out.getvalue()


def blocks_by_row(text: str, header: bool = True):
    """[(row fields, the block under it)] of a --pretty text output"""
    lines = text.split("\n")
    assert lines[-1] == ""
    lines = lines[1 if header else 0:-1]
    out = []
    for ln in lines:
        if ln.startswith("#"):
            out[-1][1].append(ln)
        else:
            out.append((ln.split("\t"), []))
    return [(f, "".join(b + "\n" for b in blk)) for f, blk in out]


# ---- 10. the reference's bytes through the whole stack

def test_forward_golden_from_the_cli(tmp_path):
    from ipcr_amd import cli
    fa = tmp_path / "a.fa"
    fa.write_text(">s\n" + "AAA" + "C" * 16 + "AAA" + "\n")
    rows = blocks_by_row(run(cli, ["-f", "AAA", "-r", "TTT", "--no-self", "--pretty", str(fa)]))
    hit = [blk for f, blk in rows if (f[3], f[4], f[6]) == ("0", "22", "forward")]
    assert hit == [golden("forward")]
    assert all(blk.startswith("# 5'-") and blk.endswith("#\n") for _, blk in rows)


def test_revcomp_golden_from_the_cli(tmp_path):
    from ipcr_amd import cli
    fa = tmp_path / "b.fa"
    fa.write_text(">s\n" + "C" * 10 + "ACGT" + "C" * 22 + "ACGT" + "C" * 24 + "\n")
    rows = blocks_by_row(run(cli, ["-f", "ACGT", "-r", "ACGT", "--pretty", str(fa)]))
    hit = [(f[6], blk) for f, blk in rows if (f[3], f[4]) == ("10", "40")]
    assert {t for t, _ in hit} == {"forward", "revcomp"}
    assert all(blk == golden("revcomp") for _, blk in hit)


def test_probe_plus_golden_from_the_cli(tmp_path):
    from ipcr_amd import cli
    fa = tmp_path / "c.fa"
    fa.write_text(">s\n" + "TCAG" + "A" * 8 + "GTACGT" + "A" * 18 + "GATC" + "\n")
    rows = blocks_by_row(run(cli, ["-f", "TCAG", "-r", "GATC", "--probe", "GTACGT", "--pretty", str(fa)]))
    hit = [blk for f, blk in rows if (f[3], f[4], f[6]) == ("0", "40", "forward")]
    assert hit == [golden("probe_plus")]


# ---- 11. the three drivers

FWD, REV = "ACGTTGCATGCARGCTTAGC", "GGCCTTAAGGCCATAYCGTATG"      # IUPAC codes inside, 20 and 22 nt
IN_F, IN_R = "TTGACCGATTAC", "CCGGTTAACGGA"
PROBE = "GATTACAGGTCATGCAA"
CLI_CFG = dict(max_mm=1, terminal_window=3, max_len=2000, hit_cap=10000, seed_len=12)


def acgt(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def concrete(primer: str, rng) -> str:
    pick = {"R": "AG", "Y": "CT"}
    return "".join(rng.choice(pick[c]) if c in pick else c for c in primer)


def plant(s, a, ln, rng, flip=False, mm_fwd=None, mm_rev=None):
    """an amplicon of ln bases at a; flip: the other orientation (a revcomp product); mm_*: substituted positions"""
    f, r = list(concrete(FWD, rng)), list(concrete(REV, rng))
    if mm_fwd is not None:
        f[mm_fwd] = O.different_base(f[mm_fwd])
    if mm_rev is not None:
        r[mm_rev] = O.different_base(r[mm_rev])
    left, right = ("".join(r), rc("".join(f))) if flip else ("".join(f), rc("".join(r)))
    s[a:a + len(left)] = left
    s[a + ln - len(right):a + ln] = right


def make_records(rng):
    a = list(acgt(rng, 30_000))
    plant(a, 1500, 300, rng)
    a[1600:1600 + len(PROBE)] = PROBE
    a[1540:1552] = IN_F
    a[1700:1712] = rc(IN_R)
    plant(a, 6000, 700, rng, mm_fwd=2)
    a[6300:6300 + len(PROBE)] = rc(PROBE)                           # the probe on the minus strand
    plant(a, 11_000, 450, rng, flip=True)
    a[11_200:11_200 + len(PROBE)] = PROBE
    plant(a, 16_000, 1200, rng, flip=True, mm_rev=4)
    plant(a, 22_000, 90, rng, mm_fwd=5, mm_rev=1)
    a[22_030:22_030 + len(PROBE)] = PROBE
    b = list(acgt(rng, 5000))
    plant(b, 3000, 520, rng)
    left = concrete(FWD, rng)                                        # across the origin: found with --circular only
    b[4900:4920] = left
    b[100:122] = rc(concrete(REV, rng))
    b[4950:4950 + len(PROBE)] = PROBE
    c = list(acgt(rng, 12_000))
    plant(c, 4000, 260, rng, mm_rev=3)                               # across the column edge at 4096
    return [("chrA", "".join(a)), ("plasmid", "".join(b)), ("chrC", "".join(c))]


def write_fa(path, recs):
    with open(path, "w") as fh:
        for name, seq in recs:
            fh.write(f">{name} some description\n")
            for i in range(0, len(seq), 70):
                fh.write(seq[i:i + 70] + "\n")


def with_self(pairs):
    out = list(pairs)
    for p in pairs:
        out.append(O.Pair(p.id + "+A:self", p.forward, p.forward))
        out.append(O.Pair(p.id + "+B:self", p.reverse, p.reverse))
    return out


def outer_rows(path, recs, pairs, circular=False, cfg=CLI_CFG):
    """(path, product with the sites sliced here, amplicon) in emission order: products from the oracle"""
    from ipcr_amd import engine
    rows = []
    for name, seq in recs:
        for w in O.simulate_batch(O.Config(circular=circular, **cfg), seq.encode(), pairs):
            pair = next(p for p in pairs if p.id == w.experiment_id)
            fp, rp = (pair.forward, pair.reverse) if w.type == "forward" else (pair.reverse, pair.forward)
            p = engine.Product(w.experiment_id, name, w.start, w.end, w.length, w.type, w.fwd_mm, w.rev_mm,
                               tuple(w.fwd_idx), tuple(w.rev_idx), FwdPrimer=fp, RevPrimer=rp)
            p.FwdSite = seq[w.start:w.start + len(fp)]
            p.RevSite = rc(seq[w.end - len(rp):w.end])
            amp = seq[w.start:w.end] if w.start <= w.end else seq[w.start:] + seq[:w.end]
            rows.append((path, p, amp))
    return rows


def render_ipcr(rows, sort, probe=None, pretty_on=True):
    from ipcr_amd import cli, pretty
    if sort:
        rows = sorted(rows, key=lambda t: cli.product_sort_key(t[0], t[1]))
    out = [cli.TSV_HEADER_PROBE if probe else cli.TSV_HEADER]
    text = ""
    for path, p, amp in rows:
        line = cli.format_row(path, p)
        block = pretty.render_product(p)
        if probe:
            h = O.best_hit(amp, probe, 0)
            if not h.found:
                continue
            line += "\t" + "\t".join(["probe", probe, "true", h.strand, str(h.pos), str(h.mm), h.site])
            block = pretty.render_annotated(p, pretty.ProbeAnnotation(Name="probe", Seq=probe, Found=True, Strand=h.strand,
                                                                      Pos=h.pos, MM=h.mm, Site=h.site))
        text += line + "\n" + (block if pretty_on else "")
    return out[0] + "\n" + text


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pretty")
    recs = make_records(random.Random(31))
    write_fa(d / "g.fa", recs)
    return str(d / "g.fa"), recs


def test_ipcr_pretty(files, monkeypatch):
    from ipcr_amd import cli
    fa, recs = files
    pairs = with_self([O.Pair("manual", FWD, REV, 0, 2000)])
    args = ["-f", FWD, "-r", REV, "-m", "1"]
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    rows = outer_rows(fa, recs, pairs)
    assert len(rows) >= 7 and {r[1].Type for r in rows} == {"forward", "revcomp"}
    assert any(r[1].FwdMM for r in rows) and any(r[1].RevMM for r in rows)
    want = render_ipcr(rows, False)
    assert "¦" in want
    assert run(cli, args + ["--pretty", fa]) == want
    assert run(cli, args + ["--pretty", "--sort", fa]) == render_ipcr(rows, True)
    # without --pretty: what the parent wrote; other formats accept the flag and ignore it
    assert run(cli, args + [fa]) == render_ipcr(rows, False, pretty_on=False)
    assert run(cli, args + ["--pretty", "-o", "jsonl", fa]) == run(cli, args + ["-o", "jsonl", fa])
    assert run(cli, args + ["--pretty", "-o", "fasta", fa]) == run(cli, args + ["-o", "fasta", fa])
    for stream in ("", "1"):                              # both chunk paths
        monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", stream)
        assert run(cli, args + ["--pretty", "--sort", "--chunk-size", "4000", fa]) == render_ipcr(rows, True), stream
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    circ = outer_rows(fa, recs, pairs, circular=True)
    wrap = [r for r in circ if r[1].Start > r[1].End]
    assert len(wrap) == 1 and wrap[0][1].SequenceID == "plasmid"
    assert run(cli, args + ["--pretty", "--circular", fa]) == render_ipcr(circ, False)


def test_ipcr_probe_pretty(files, monkeypatch):
    from ipcr_amd import cli
    fa, recs = files
    pairs = with_self([O.Pair("manual", FWD, REV, 0, 2000)])
    args = ["-f", FWD, "-r", REV, "-m", "1", "--probe", PROBE]
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    rows = outer_rows(fa, recs, pairs)
    want = render_ipcr(rows, False, probe=PROBE)
    assert want.count("probe (+)") >= 2 and want.count("probe (-)") >= 1
    assert run(cli, args + ["--pretty", fa]) == want
    assert run(cli, args + ["--pretty", "--sort", fa]) == render_ipcr(rows, True, probe=PROBE)
    assert run(cli, args + [fa]) == render_ipcr(rows, False, probe=PROBE, pretty_on=False)
    for stream in ("", "1"):
        monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", stream)
        assert run(cli, args + ["--pretty", "--sort", "--chunk-size", "4000", fa]) == render_ipcr(rows, True, probe=PROBE), stream
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    circ = outer_rows(fa, recs, pairs, circular=True)
    want = render_ipcr(circ, False, probe=PROBE)
    assert 'sequence_id' in want and any(p.Start > p.End and O.best_hit(amp, PROBE, 0).found for _, p, amp in circ)
    assert run(cli, args + ["--pretty", "--circular", fa]) == want


def render_nested(rows, inner_pairs, sort, pretty_on=True):
    from ipcr_amd import nested, nested_cli, pretty
    out = []
    for path, p, amp in rows:
        hits = O.simulate_batch(O.Config(max_mm=1, terminal_window=3, seed_len=12), amp.encode(), inner_pairs)
        if hits:
            h = sorted(hits, key=lambda h: (h.fwd_mm + h.rev_mm, -h.length, h.start, h.end, h.experiment_id))[0]
            np = nested.NestedProduct(p, True, h.experiment_id, h.start, h.end, h.length, h.type, h.fwd_mm, h.rev_mm)
        else:
            np = nested.NestedProduct(p, False)
        out.append((path, np, amp))
    if sort:
        out = nested_cli.sort_rows(out)
    return nested_cli.TSV_HEADER_NESTED + "\n" + "".join(
        nested_cli.format_row(path, np) + "\n" + (pretty.render_product(np.Product) if pretty_on else "")
        for path, np, _ in out), out


def test_ipcr_nested_pretty(files, monkeypatch):
    from ipcr_amd import nested_cli
    fa, recs = files
    outer = with_self([O.Pair("outer", FWD, REV, 0, 2000)])
    inner = with_self([O.Pair("inner", IN_F, IN_R)])
    args = ["-f", FWD, "-r", REV, "-F", IN_F, "-R", IN_R, "-m", "1"]
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    rows = outer_rows(fa, recs, outer)
    want, nps = render_nested(rows, inner, False)
    assert any(np.InnerFound for _, np, _ in nps) and not all(np.InnerFound for _, np, _ in nps)
    assert run(nested_cli, args + ["--pretty", fa]) == want
    assert run(nested_cli, args + ["--pretty", "--sort", fa]) == render_nested(rows, inner, True)[0]
    assert run(nested_cli, args + [fa]) == render_nested(rows, inner, False, pretty_on=False)[0]
    assert run(nested_cli, args + ["--pretty", "-o", "jsonl", fa]) == run(nested_cli, args + ["-o", "jsonl", fa])
    for stream in ("", "1"):
        monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", stream)
        assert run(nested_cli, args + ["--pretty", "--sort", "--chunk-size", "4000", fa]) == render_nested(rows, inner, True)[0], stream
    monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "")
    circ = outer_rows(fa, recs, outer, circular=True)
    assert any(p.Start > p.End for _, p, _ in circ)
    assert run(nested_cli, args + ["--pretty", "--circular", fa]) == render_nested(circ, inner, False)[0]
