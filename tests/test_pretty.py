"""ipcr_amd.pretty against the reference's own recorded output (tests/golden/pretty/*.golden, copied unchanged from the
reference's internal/pretty/testdata) and against cases derived from its source; flag parsing of --pretty.  No GPU."""
import json
import os
from types import SimpleNamespace

import pytest

from ipcr_amd import pretty

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretty")


def product(**kw):
    base = dict(FwdPrimer="", RevPrimer="", FwdSite="", RevSite="", Length=0, Start=0, End=0, Type="forward", FwdMM=0,
                RevMM=0, FwdMismatchIdx=(), RevMismatchIdx=())
    base.update(kw)
    return SimpleNamespace(**base)


def _cases():
    with open(os.path.join(GOLDEN, "cases.json"), encoding="utf-8") as fh:
        return json.load(fh)["cases"]


def _render(case) -> str:
    p = product(**case["product"])
    if case["probe"] is None:
        return pretty.render_product(p)
    return pretty.render_annotated(p, pretty.ProbeAnnotation(**case["probe"]))


# ---- 1. the reference's golden files, byte for byte

@pytest.mark.parametrize("name", ["forward", "revcomp", "probe_plus", "probe_minus", "probe_minus_near_forward"])
def test_reference_golden_bytes(name):
    case = next(c for c in _cases() if c["name"] == name)
    with open(os.path.join(GOLDEN, name + ".golden"), "rb") as fh:
        want = fh.read()
    assert _render(case).encode("utf-8") == want


def test_golden_files_are_the_reference_s():
    """the five files are 1806 bytes in all (what the reference's checkout holds)"""
    sizes = {n: os.path.getsize(os.path.join(GOLDEN, n + ".golden")) for n in
             ("forward", "revcomp", "probe_plus", "probe_minus", "probe_minus_near_forward")}
    assert sizes == {"forward": 147, "revcomp": 177, "probe_plus": 320, "probe_minus": 640, "probe_minus_near_forward": 522}


# ---- 2. pretty_test.go:149-179 and defaults_snapshot_test.go

def test_minus_probe_unequal_primer_lengths_equal_genomic_line_widths():
    p = product(FwdPrimer="GTTTACCCATATCTTTGACGCTCTTA", RevPrimer="GGAAAGACATATCCCAATACAGCAA",
                FwdSite="GTTTACCCATATCTTTGACGCTCTTA", RevSite="GGAAAGACATATCCCAATACAGCAA",
                Length=68, Start=861241, End=861309, Type="revcomp")
    ann = pretty.ProbeAnnotation(Name="probe", Seq="TCGGTGCTGGAAGAA", Found=True, Strand="-", Pos=27, MM=0,
                                 Site="TTCTTCCAGCACCGA")
    assert (len(p.FwdPrimer), len(p.RevPrimer)) == (26, 25)
    got = pretty.render_annotated(p, ann)
    plus = [ln for ln in got.split("\n") if "# (+)" in ln]
    minus = [ln for ln in got.split("\n") if "# (-)" in ln]
    assert len(plus) == 1 and len(minus) == 1, got
    a, b = plus[0][:-len(" # (+)")], minus[0][:-len(" # (-)")]
    assert plus[0].endswith(" # (+)") and minus[0].endswith(" # (-)")
    assert len(a.encode()) == len(b.encode()), got


def test_default_options_stable():
    assert (pretty.DOT_GLYPH, pretty.EXACT_GLYPH, pretty.PARTIAL_GLYPH) == (".", "|", "¦")
    assert pretty.MAX_GAP == 95
    assert pretty.PARTIAL_GLYPH.encode("utf-8") == b"\xc2\xa6"          # two bytes: what len() counts in the source


# ---- 3. byte length against character count (derived from the source, not reference output)

def test_plus_probe_bars_overlap_by_bytes_not_by_characters():
    """Derived from the source, not reference output (pretty.go:518-546).  aLen 8, bLen 4, Length 60: interior = inner =
    48, innerPlus 48, innerMinus 52.  Probe on + at Pos 14: off 6, scaled 6 * 47 // 47 = 6, column 3 + 8 + 6 = 17.
    Sequence row: the probe block starts at column 14 = len("5'-RYMKACGT-3'"): no overlap.  Bars row: the forward bars
    block "¦¦¦¦||||-->" is 11 characters (columns 3..13) but len() gives 4 * 2 + 4 + 3 = 15 bytes (3..17), and the probe
    bars start at 17 < 18: overlap, so the probe goes on rows of its own."""
    p = product(FwdPrimer="RYMKACGT", FwdSite="ACAGACGT", RevPrimer="GATC", RevSite="GATC", Length=60, Start=0, End=60)
    ann = pretty.ProbeAnnotation(Name="probe", Seq="GTACGT", Found=True, Strand="+", Pos=14, MM=0, Site="GTACGT")
    want = ("# 5'-RYMKACGT-3'\n"
            "#    ¦¦¦¦||||-->\n"
            "#               5'-GTACGT-3' probe (+)\n"
            "#                  ||||||\n"
            "# 5'-ACAGACGT......GTACGT....................................-3' # (+)\n"
            "# 3'-....................................................CTAG-5' # (-)\n"
            "#                                                     <--||||\n"
            "#                                                     3'-CTAG-5'\n"
            "# probe \"probe\" (+) pos=14 mm=0 site=GTACGT fwd_mm=0@[] rev_mm=0@[]\n"
            "#\n")
    assert pretty.render_annotated(p, ann) == want
    # the same probe under an all-ACGT primer of the same length shares the first two rows (bytes == characters): its
    # block starts at column 14, directly behind the forward primer's, and its bars at 17, behind the arrow (3..13)
    q = product(FwdPrimer="ACAGACGT", FwdSite="ACAGACGT", RevPrimer="GATC", RevSite="GATC", Length=60, Start=0, End=60)
    got = pretty.render_annotated(q, ann).split("\n")
    assert got[0] == "# 5'-ACAGACGT-3'5'-GTACGT-3' probe (+)"
    assert got[1] == "#    ||||||||-->   ||||||"


# ---- 4. missing sites, overlapping primers, mismatch blanks

def test_sites_missing_block():
    want = "# (pretty not available: sites missing)\n\n"
    p = product(FwdPrimer="ACGT", RevPrimer="ACGT", Length=30)
    assert pretty.render_product(p) == want
    assert pretty.render_annotated(p, pretty.ProbeAnnotation(Name="x")) == want
    assert pretty.render_product(product(FwdPrimer="ACGT", RevPrimer="ACGT", FwdSite="ACGT", Length=30)) == want


def test_overlapping_primers_interior_clamped():
    """Length < aLen + bLen: interior is clamped to 0 (pretty.go:342-345); inner 0, innerMinus = aLen + 5 = 11,
    innerPlus = bLen + 5 = 11: both rows 6 + 11 wide.  Derived from the source."""
    p = product(FwdPrimer="ACGTAC", FwdSite="ACGTAC", RevPrimer="GTACGT", RevSite="GTACGT", Length=8, Start=0, End=8)
    want = ("# 5'-ACGTAC-3'\n"
            "#    ||||||-->\n"
            "# 5'-ACGTAC...........-3' # (+)\n"
            "# 3'-...........CATGCA-5' # (-)\n"
            "#            <--||||||\n"
            "#            3'-TGCATG-5'\n"
            "#\n")
    assert pretty.render_product(p) == want
    # a found probe has no interior to sit in: no overlay, the summary line only
    ann = pretty.ProbeAnnotation(Name="probe", Seq="GT", Found=True, Strand="+", Pos=2, MM=0, Site="GT")
    got = pretty.render_annotated(p, ann).split("\n")
    assert got[:6] == want.split("\n")[:6]
    assert got[6] == '# probe "probe" (+) pos=2 mm=0 site=GT fwd_mm=0@[] rev_mm=0@[]'
    assert got[7:] == ["#", ""]


def test_mismatch_indices_blank_the_bars():
    """FwdMismatchIdx blanks its own column; RevMismatchIdx is in primer 5'->3' coordinates and the bars are reversed
    for display (pretty.go:394): index 1 of a 5 nt primer is the fourth bar from the left.  Derived from the source."""
    p = product(FwdPrimer="ACGTR", FwdSite="ATGTA", RevPrimer="GGYCC", RevSite="GAYCC", Length=30, Start=0, End=30,
                FwdMM=1, RevMM=1, FwdMismatchIdx=(1,), RevMismatchIdx=(1,))
    got = pretty.render_product(p).split("\n")
    assert got[1] == "#    | ||¦-->"
    assert got[3].endswith("CTRGG-5' # (-)")                            # complement of RevSite, not reversed
    assert got[4].endswith("<--||¦ |")
    assert got[5].endswith("3'-CCYGG-5'")
    ann = pretty.ProbeAnnotation(Name="p1", Found=False)
    last = pretty.render_annotated(p, ann).split("\n")
    assert last[-3] == '# probe "p1" NOT FOUND fwd_mm=1@[1] rev_mm=1@[1]'
    assert last[1] == got[1] and last[4].rstrip() == got[4].rstrip()


def test_probe_bars_use_base_match():
    """a probe position that does not match its site is blank, an IUPAC probe base gives the partial glyph
    (pretty.go:196-221)"""
    p = product(FwdPrimer="TCAG", FwdSite="TCAG", RevPrimer="GATC", RevSite="GATC", Length=40, Start=0, End=40)
    ann = pretty.ProbeAnnotation(Name="probe", Seq="GTRCGA", Found=True, Strand="+", Pos=12, MM=1, Site="GTACGT")
    got = pretty.render_annotated(p, ann).split("\n")
    assert got[0] == "# 5'-TCAG-3'  5'-GTRCGA-3' probe (+)"
    assert got[1] == "#    ||||-->     ||¦||"


# ---- 5. flags

def test_pretty_flag_both_parsers_and_need_sites():
    from ipcr_amd import cli, nested_cli, pipeline
    o = cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "--pretty", "x.fa"])
    assert o.pretty and pipeline.want_pretty(o)
    assert not cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "x.fa"]).pretty
    o = cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "--pretty", "--output", "jsonl", "x.fa"])
    assert o.pretty and not pipeline.want_pretty(o)
    assert cli.engine_config(o).NeedSites is False
    o = cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "--pretty", "--output", "fasta", "x.fa"])
    assert cli.engine_config(o).NeedSites is False
    o = cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "--pretty", "x.fa"])
    assert cli.engine_config(o).NeedSites is True
    assert cli.engine_config(cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "x.fa"])).NeedSites is False
    o = nested_cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "-F", "AC", "-R", "GT", "--pretty", "x.fa"])
    assert o.pretty and pipeline.want_pretty(o)
    o = nested_cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "-F", "AC", "-R", "GT", "--pretty", "-o", "jsonl", "x.fa"])
    assert o.pretty and not pipeline.want_pretty(o)
