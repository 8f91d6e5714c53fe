"""The `--pretty` alignment block: internal/pretty/pretty.go restated with its DefaultOptions (MaxGap 95, probe inline,
probe bars and sequence row on, caret off, glyphs | ¦ .).

Host-side presentation only.  Two things in the source decide the layout and are kept as they are:

* Go's len(string) counts BYTES while putAt places RUNES.  `¦` takes two bytes in UTF-8, so every len() of a bars string
  that holds one (a primer or probe with an IUPAC code) is larger than its width on the screen: `_blen` below stands where
  the source says len(), character positions where it goes through putAt.
* With a probe found on the minus strand both genomic rows are widened by the forward primer's length
  (pretty.go:475-489).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

MAX_GAP = 95
EXACT_GLYPH = "|"
PARTIAL_GLYPH = "¦"        # ¦
DOT_GLYPH = "."
MIN_INTER_PRIMER_GAP = 5
LINE_PREFIX = "# "
MISSING = LINE_PREFIX + "(pretty not available: sites missing)\n\n"   # pretty.go:326-330

_PREFIX_PLUS, _SUFFIX_PLUS, _PREFIX_MINUS, _SUFFIX_MINUS = "5'-", "-3'", "3'-", "-5'"
_ARROW_RIGHT, _ARROW_LEFT = "-->", "<--"

# core/primer/rc.go:8-24
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
               "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}
# core/primer/iupac.go:6-58 (A 1, C 2, G 4, T 8; lower case as upper, anything else 0)
_MASK = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11,
         "V": 7, "N": 15}


@dataclass
class ProbeAnnotation:
    """pretty.ProbeAnnotation -- pretty.go:11-19; Pos is 0-based in the amplicon, plus orientation"""
    Name: str = ""
    Seq: str = ""
    Found: bool = False
    Strand: str = ""
    Pos: int = 0
    MM: int = 0
    Site: str = ""


def _blen(s: str) -> int:
    """Go's len(string): the UTF-8 byte length"""
    return len(s.encode("utf-8"))


def comp5to3(s: str) -> str:
    """the complement (not reversed) of a 5'->3' string -- pretty.go:75-86; RevComp panics on a byte outside the
    upper-case IUPAC alphabet, this raises ValueError"""
    try:
        return "".join(_COMPLEMENT[c] for c in s)
    except KeyError as e:
        raise ValueError(f"invalid reverse-complement base {e.args[0]!r}; expected normalized uppercase IUPAC DNA")


def _is_acgt(c: str) -> bool:
    return c in ("A", "C", "G", "T")


def _base_match(g: str, p: str) -> bool:
    """primer.BaseMatch -- core/primer/iupac.go:62-67: the genome base must be an upper-case A, C, G or T"""
    return _is_acgt(g) and bool(_MASK.get(p.upper(), 0) & _MASK[g])


def match_line_ambig(primer_seq: str, site: str, mism_idx: Sequence[int]) -> str:
    """bars under a primer -- pretty.go:91-117: blank at a mismatch, | under A/C/G/T, ¦ under an IUPAC code"""
    n = min(len(primer_seq), len(site))
    bad = set(mism_idx)
    return "".join(" " if i in bad else (EXACT_GLYPH if _is_acgt(primer_seq[i]) else PARTIAL_GLYPH) for i in range(n))


def scale_pos(off: int, interior: int, inner: int) -> int:
    """pretty.go:119-130"""
    if interior <= 1 or inner <= 1:
        return 0
    off = min(max(off, 0), interior - 1)
    return (off * (inner - 1)) // (interior - 1)


def _put_at(line: List[str], col: int, text: str) -> List[str]:
    """pretty.go:156-181, over characters"""
    if not text:
        return line
    chars = list(text)
    if col < 0:
        if -col >= len(chars):
            return line
        chars = chars[-col:]
        col = 0
    need = col + len(chars)
    if need > len(line):
        line = line + [" "] * (need - len(line))
    line[col:col + len(chars)] = chars
    return line


def _render_segments(segs: Sequence[Tuple[int, str]]) -> str:
    """pretty.go:148-154"""
    line: List[str] = []
    for col, text in segs:
        line = _put_at(line, col, text)
    return "".join(line).rstrip(" ")


def _probe_match_line(probe_seq: str, site: str) -> str:
    """pretty.go:196-221"""
    n = min(len(probe_seq), len(site))
    return "".join(" " if not _base_match(site[i], probe_seq[i]) else
                   (EXACT_GLYPH if _is_acgt(probe_seq[i]) else PARTIAL_GLYPH) for i in range(n))


def _ranges_overlap(a_start: int, a_len: int, b_start: int, b_len: int) -> bool:
    if a_len <= 0 or b_len <= 0:
        return False
    return a_start < b_start + b_len and b_start < a_start + a_len


def _probe_overlay(ann: ProbeAnnotation, a_len: int, interior: int, inner: int, plus_offset: int, minus_offset: int):
    """pretty.go:245-313: (strand, column, site segment, probe segment, bars) or None"""
    if not ann.Found or not ann.Site or interior <= 0 or inner <= 0:
        return None
    strand = "-" if ann.Strand == "-" else "+"
    site = ann.Site
    probe_seq = ann.Seq or site
    if strand == "-":
        site = comp5to3(site)
        probe_seq = probe_seq[::-1]
    n = min(len(site), len(probe_seq))
    site, probe_seq = site[:n], probe_seq[:n]
    start = ann.Pos
    if start < a_len:
        clip = a_len - start
        if clip >= len(site) or clip >= len(probe_seq):
            return None
        site, probe_seq = site[clip:], probe_seq[clip:]
        start = a_len
    if start >= a_len + interior:
        return None
    scaled = scale_pos(start - a_len, interior, inner)
    slot = inner - scaled
    if slot <= 0:
        return None
    site = site[:slot]
    probe_seq = probe_seq[:len(site)]
    if not site or not probe_seq:
        return None
    col = (minus_offset if strand == "-" else plus_offset) + scaled
    return strand, col, site, probe_seq, _probe_match_line(probe_seq, site)


def _geometry(p):
    """the widths both renderers start from -- pretty.go:341-366"""
    a_len, b_len = len(p.FwdPrimer), len(p.RevPrimer)
    interior = max(p.Length - a_len - b_len, 0)
    inner = min(MAX_GAP, interior)
    inner_minus = max(inner, a_len + MIN_INTER_PRIMER_GAP)
    inner_plus = max(inner, b_len + MIN_INTER_PRIMER_GAP)
    cont_plus, cont_minus = a_len + inner_plus, inner_minus + b_len
    if cont_minus > cont_plus:
        inner_plus += cont_minus - cont_plus
    elif cont_plus > cont_minus:
        inner_minus += cont_plus - cont_minus
    return a_len, b_len, interior, inner_plus, inner_minus


def _sites_missing(p) -> bool:
    return not (p.FwdPrimer and p.RevPrimer and p.FwdSite and p.RevSite)


def render_product(p) -> str:
    """pretty.RenderProduct -- pretty.go:316-412: the block under a product's row, no probe"""
    if _sites_missing(p):
        return MISSING
    _, _, _, inner_plus, inner_minus = _geometry(p)
    site_start = len(_PREFIX_MINUS) + inner_minus
    rev_bars = match_line_ambig(p.RevPrimer, p.RevSite, p.RevMismatchIdx)[::-1]
    lines = [
        _PREFIX_PLUS + p.FwdPrimer + _SUFFIX_PLUS,
        " " * len(_PREFIX_PLUS) + match_line_ambig(p.FwdPrimer, p.FwdSite, p.FwdMismatchIdx) + _ARROW_RIGHT,
        _PREFIX_PLUS + p.FwdSite + DOT_GLYPH * inner_plus + _SUFFIX_PLUS + " # (+)",
        _PREFIX_MINUS + DOT_GLYPH * inner_minus + comp5to3(p.RevSite) + _SUFFIX_MINUS + " # (-)",
        " " * max(site_start - len(_ARROW_LEFT), 0) + _ARROW_LEFT + rev_bars,
        " " * max(site_start - len(_PREFIX_MINUS), 0) + _PREFIX_MINUS + p.RevPrimer[::-1] + _SUFFIX_MINUS,
    ]
    return "".join(LINE_PREFIX + ln + "\n" for ln in lines) + "#\n"


def _probe_label(name: str) -> str:
    return name or "probe"


def _go_quote(s: str) -> str:
    """fmt's %q for the names this prints: strconv.Quote of printable text"""
    out = ['"']
    for ch in s:
        if ch in ('"', "\\"):
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\r":
            out.append("\\r")
        elif ord(ch) < 0x20 or ord(ch) == 0x7F:
            out.append("\\x%02x" % ord(ch))
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def _ints_csv(a: Sequence[int]) -> str:
    return ",".join(str(v) for v in a)


def render_annotated(p, ann: ProbeAnnotation) -> str:
    """pretty.RenderAnnotated -- pretty.go:420-647: the block with the probe overlay"""
    if _sites_missing(p):
        return MISSING
    a_len, _, interior, inner_plus, inner_minus = _geometry(p)
    minus_probe_mode = ann.Found and ann.Strand == "-" and len(ann.Site) > 0
    plus_interior_len, minus_interior_len, minus_probe_offset = inner_plus, inner_minus, len(_PREFIX_MINUS)
    if minus_probe_mode:                                                # both genomic rows widened by a_len
        plus_interior_len = inner_plus + a_len
        minus_interior_len = a_len + inner_minus
        minus_probe_offset = len(_PREFIX_MINUS) + a_len
    plus_interior = DOT_GLYPH * plus_interior_len
    minus_interior = DOT_GLYPH * minus_interior_len
    plus_interior_start = len(_PREFIX_PLUS) + a_len
    minus_interior_start = len(_PREFIX_MINUS)
    ov_plus = _probe_overlay(ann, a_len, interior, inner_plus, plus_interior_start, minus_probe_offset)
    ov_minus = None
    if ov_plus is not None and ov_plus[0] == "-":
        ov_minus = _probe_overlay(ann, a_len, interior, inner_minus, plus_interior_start, minus_probe_offset)
        ov_plus = None

    if ov_plus is not None:                                             # ShowProbeInline
        plus_interior = _render_segments([(0, plus_interior), (ov_plus[1] - plus_interior_start, ov_plus[2])])
    if ov_minus is not None:
        minus_interior = _render_segments([(0, minus_interior), (ov_minus[1] - minus_interior_start, ov_minus[2])])

    fwd_seq_block = _PREFIX_PLUS + p.FwdPrimer + _SUFFIX_PLUS
    fwd_bars_block = match_line_ambig(p.FwdPrimer, p.FwdSite, p.FwdMismatchIdx) + _ARROW_RIGHT
    top_seq, top_bars = [(0, fwd_seq_block)], [(len(_PREFIX_PLUS), fwd_bars_block)]
    extra_top_seq, extra_top_bars = [], []
    if ov_plus is not None:
        _, col, _, probe_seg, bars = ov_plus
        probe_seq_block = _PREFIX_PLUS + probe_seg + _SUFFIX_PLUS + " " + _probe_label(ann.Name) + " (+)"
        probe_seq_col = col - len(_PREFIX_PLUS)
        # byte lengths, as the source's len() gives them (pretty.go:529-530)
        overlaps = (_ranges_overlap(probe_seq_col, _blen(probe_seq_block), 0, _blen(fwd_seq_block)) or
                    _ranges_overlap(col, _blen(bars), len(_PREFIX_PLUS), _blen(fwd_bars_block)))
        if overlaps:
            extra_top_seq.append((probe_seq_col, probe_seq_block))
            extra_top_bars.append((col, bars))
        else:
            top_seq.append((probe_seq_col, probe_seq_block))
            top_bars.append((col, bars))

    site_start = len(_PREFIX_MINUS) + minus_interior_len
    rev_bars = match_line_ambig(p.RevPrimer, p.RevSite, p.RevMismatchIdx)[::-1]
    arrow_start_col = max(site_start - len(_ARROW_LEFT), 0)
    right_block = _PREFIX_MINUS + p.RevPrimer[::-1] + _SUFFIX_MINUS
    right_start_col = max(arrow_start_col + len(_ARROW_LEFT) - len(_PREFIX_MINUS), 0)
    bottom_bars, bottom_seq = [(arrow_start_col, _ARROW_LEFT + rev_bars)], [(right_start_col, right_block)]
    extra_bottom_bars, extra_bottom_seq = [], []
    if ov_minus is not None:
        _, col, _, probe_seg, bars = ov_minus
        label = _probe_label(ann.Name) + " (-) "
        probe_seq_block = label + _PREFIX_MINUS + probe_seg + _SUFFIX_MINUS
        probe_seq_col = col - _blen(label) - len(_PREFIX_MINUS)
        overlaps = (_ranges_overlap(probe_seq_col, _blen(probe_seq_block), right_start_col, _blen(right_block)) or
                    _ranges_overlap(col, _blen(bars), arrow_start_col, len(_ARROW_LEFT) + _blen(rev_bars)))   # :572-573
        if overlaps:
            extra_bottom_bars.append((col, bars))
            extra_bottom_seq.append((probe_seq_col, probe_seq_block))
        else:
            bottom_bars.append((col, bars))
            bottom_seq.append((probe_seq_col, probe_seq_block))

    lines = [_render_segments(top_seq), _render_segments(top_bars)]
    if extra_top_seq or extra_top_bars:
        lines += [_render_segments(extra_top_seq), _render_segments(extra_top_bars)]
    lines.append(_PREFIX_PLUS + p.FwdSite + plus_interior + _SUFFIX_PLUS + " # (+)")
    lines.append(_PREFIX_MINUS + minus_interior + comp5to3(p.RevSite) + _SUFFIX_MINUS + " # (-)")
    if extra_bottom_bars or extra_bottom_seq:
        lines += [_render_segments(extra_bottom_bars), _render_segments(extra_bottom_seq)]
    lines += [_render_segments(bottom_bars), _render_segments(bottom_seq)]
    mm = "fwd_mm=%d@[%s] rev_mm=%d@[%s]" % (p.FwdMM, _ints_csv(p.FwdMismatchIdx), p.RevMM, _ints_csv(p.RevMismatchIdx))
    if ann.Found:
        lines.append("probe %s (%s) pos=%d mm=%d site=%s %s" % (_go_quote(ann.Name), ann.Strand, ann.Pos, ann.MM, ann.Site, mm))
    else:
        lines.append("probe %s NOT FOUND %s" % (_go_quote(ann.Name), mm))
    return "".join(LINE_PREFIX + ln + "\n" for ln in lines) + "#\n"
