"""Minimal `ipcr` / `ipcr-probe` / `ipcr-multiplex` driver over the HIP engine.

Only what sits directly either side of the scan path ("next" 1 and 2):
FASTA -> resident tiles, the collector's total product order, and the text/TSV rows -- with the
reference's flag names and defaults (internal/clibase/common.go:61-110) so outputs can be
diffed against `ipcr`.  --products (JSONL `seq`) and --output fasta carry the amplicon bytes, read exactly from the
resident genome (ipcr_genome_read_windows).  The data paths (resident, --chunk-size, streamed chunks) are `ipcr_amd.pipeline`.  --pretty writes the alignment block of
`ipcr_amd.pretty` under every text row, from sites the device read (ipcr_product_sites).  Thermo scoring and the JSON
array are out of scope; nested PCR is `ipcr_amd.nested_cli`.

    python -m ipcr_amd.cli -f AGAGTTTGATCMTGGCTCAG -r TACGGYTACCTTGTTAYGACTT --mismatches 0 demo.fa
"""
from __future__ import annotations

import argparse
import sys
from typing import List, Optional, Sequence

from . import engine, pipeline, pretty, primer

TSV_HEADER = ("source_file\tsequence_id\texperiment_id\tstart\tend\tlength\ttype\tfwd_mm\trev_mm"
              "\tfwd_mm_i\trev_mm_i")                                   # internal/output/common.go:5
TSV_HEADER_PROBE = TSV_HEADER + ("\tprobe_name\tprobe_seq\tprobe_found\tprobe_strand\tprobe_pos"
                                 "\tprobe_mm\tprobe_site")              # internal/probeoutput/types.go:24-26


def load_tsv(path: str) -> List[primer.Pair]:
    """primer.LoadTSV -- core/primer/loader.go:11-61"""
    out = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line[0] == "#":
                continue
            f = line.split()
            if len(f) < 3 or len(f) > 5:
                raise ValueError(f"{path}:{ln} bad field count")
            p = primer.Pair(f[0], primer.Validate(f[1]), primer.Validate(f[2]))
            if len(f) >= 4:
                p.MinProduct = int(f[3])
            if len(f) == 5:
                p.MaxProduct = int(f[4])
            out.append(p)
    return out


def ints_csv(a: Sequence[int]) -> str:  # internal/output/rows.go:10-19
    return ",".join(str(v) for v in a)


def split_chunk_suffix(seq_id: str):
    """common.SplitChunkSuffix -- internal/common/ids.go:11-27"""
    colon = seq_id.rfind(":")
    if colon == -1 or colon == len(seq_id) - 1:
        return seq_id, 0, False
    suffix = seq_id[colon + 1:]
    dash = suffix.find("-")
    if dash == -1:
        return seq_id, 0, False
    start = _atoi(suffix[:dash])
    if start is None:
        return seq_id, 0, False
    return seq_id[:colon], start, True


def _atoi(text: str):
    """strconv.Atoi (ids.go:21): optional sign, then ASCII digits only, value inside int64 -- Python's int() also
    takes surrounding blanks, '_' separators and non-ASCII digits, which would rebase IDs such as "x: 7-9" or
    "x:1_0-5" that the reference leaves alone.  None where Atoi returns an error."""
    body = text[1:] if text[:1] in ("+", "-") else text
    if not body or not all("0" <= ch <= "9" for ch in body):
        return None
    v = int(body)
    if text[:1] == "-":
        v = -v
    if v < -(1 << 63) or v > (1 << 63) - 1:
        return None
    return v


def compute_overlap(max_len: int, max_primer_len: int) -> int:
    """runutil.ComputeOverlap -- internal/runutil/runutil.go:20-31"""
    if max_len > 0:
        return max_len
    return max(max_primer_len - 1, 0)


def validate_chunking(circular: bool, chunk_size: int, max_len: int, max_primer_len: int):
    """runutil.ValidateChunking -- internal/runutil/runutil.go:33-62: (chunk, overlap, warnings)"""
    if chunk_size <= 0:
        return 0, 0, []
    if circular:
        return 0, 0, ["chunking disabled for circular templates"]
    if max_len <= 0:
        return 0, 0, ["chunking disabled: a finite effective max product length is required to compute safe overlap"]
    if chunk_size <= max_len:
        return 0, 0, [f"chunk-size ({chunk_size}) <= effective max product length ({max_len}): disabling chunking"]
    return chunk_size, compute_overlap(max_len, max_primer_len), []


class Collector:
    """The pipeline's collector goroutine -- internal/pipeline/pipeline.go:127-161: chunk-local coordinates become
    record-global ones (any ID ending ':<int>-...' counts as a chunk, ids.go:11-27), products seen in the overlap
    of two chunks are dropped by a bounded FIFO/LRU set (runutil/lru_set.go, default 200 000 keys)."""

    def __init__(self, cap: int = 0):
        from collections import OrderedDict
        self.cap = cap if cap > 0 else 200_000
        self.seen = OrderedDict()

    def add(self, source_file: str, p: engine.Product):
        base, off, ok = split_chunk_suffix(p.SequenceID)
        if not ok:
            base, off = p.SequenceID, 0
        gs, ge = p.Start + off, p.End + off
        k = (base, source_file, gs, ge, p.Type, p.ExperimentID)
        if k in self.seen:
            self.seen.move_to_end(k, last=False)
            return None
        self.seen[k] = True
        self.seen.move_to_end(k, last=False)
        if len(self.seen) > self.cap:
            self.seen.popitem(last=True)
        if ok:
            p.SequenceID, p.Start, p.End = base, gs, ge
        return p


def product_sort_key(source_file: str, p: engine.Product):
    """common.LessProduct -- internal/common/sort.go:34-78 as a sort key."""
    base, off, ok = split_chunk_suffix(p.SequenceID)
    if not ok:
        base, off = p.SequenceID, 0
    return (source_file, base, p.Start + off, p.End + off, p.Length, p.Type, p.ExperimentID, p.FwdMM, p.RevMM,
            ints_csv(p.FwdMismatchIdx), ints_csv(p.RevMismatchIdx), p.SequenceID)


def format_row(source_file: str, p: engine.Product) -> str:
    """output.FormatBaseRowTSV -- internal/output/rows.go:21-29"""
    return "\t".join([source_file, p.SequenceID, p.ExperimentID, str(p.Start), str(p.End), str(p.Length), p.Type,
                      str(p.FwdMM), str(p.RevMM), ints_csv(p.FwdMismatchIdx), ints_csv(p.RevMismatchIdx)])


def format_jsonl(source_file: str, p: engine.Product, seq: str = "") -> str:
    """One line of --output jsonl: api.ProductV1 (pkg/api/products_v1.go:6-25) as encoding/json writes it -- field
    order of the struct, zero / empty `omitempty` fields left out, compact separators, <, > and & escaped.  `seq`
    (--products) goes between rev_mm_i and source_file, left out when empty."""
    import json
    d = {"experiment_id": p.ExperimentID, "sequence_id": p.SequenceID, "start": p.Start, "end": p.End,
         "length": p.Length, "type": p.Type}
    if p.FwdMM:
        d["fwd_mm"] = p.FwdMM
    if p.RevMM:
        d["rev_mm"] = p.RevMM
    if p.FwdMismatchIdx:
        d["fwd_mm_i"] = list(p.FwdMismatchIdx)
    if p.RevMismatchIdx:
        d["rev_mm_i"] = list(p.RevMismatchIdx)
    if seq:
        d["seq"] = seq
    if source_file:
        d["source_file"] = source_file
    return go_json_escape(json.dumps(d, separators=(",", ":"), ensure_ascii=False))


def go_json_escape(text: str) -> str:
    """encoding/json's HTML escaping (the Encoder default) over what json.dumps wrote: <, > and & as \\u escapes"""
    return text.replace("<", "\\u003c").replace(">", "\\u003e").replace("&", "\\u0026")


def format_fasta(idx: int, source_file: str, p: engine.Product, seq: str) -> str:
    """One record of --output fasta -- internal/output/fasta.go:11-44 (without the final newline)."""
    return f">{p.ExperimentID}_{idx} start={p.Start} end={p.End} len={p.Length} source_file={source_file}\n{seq}"


def fasta_records(rows, sort: bool) -> List[str]:
    """--output fasta over (source_file, product, seq) rows: products with an empty sequence are skipped.  Unsorted
    (StreamFASTA) the index counts the records written; --sort (WriteFASTA) it is the position in the sorted list + 1
    (internal/writers/product.go:66-80)."""
    out, written = [], 0
    for i, (path, p, seq) in enumerate(rows):
        if not seq:
            continue
        written += 1
        out.append(format_fasta(i + 1 if sort else written, path, p, seq))
    return out


def _text(b: bytes) -> str:
    return b.decode("latin-1")  # one character per byte: bytes >= 0x80 are kept as they were loaded


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="ipcr-hip", add_help=True)
    ap.add_argument("--primers", "-p", default="")
    ap.add_argument("--forward", "-f", default="")
    ap.add_argument("--reverse", "-r", default="")
    pipeline.add_common_flags(ap, dict(choices=["text", "jsonl", "fasta"]),
                              "scan rolling chunks through ipcr_scan_chunk (0 = whole records resident)")
    ap.add_argument("--products", action="store_true", help="carry each product's sequence (JSONL field `seq`)")
    ap.add_argument("--multiplex", action="store_true", help="ipcr-multiplex self-pair rule (unique oligos)")
    ap.add_argument("--probe", "-P", default="")
    ap.add_argument("--probe-name", default="probe")
    ap.add_argument("--probe-max-mm", "-M", type=int, default=0)
    ap.add_argument("--require-probe", action=argparse.BooleanOptionalAction, default=True)
    return ap


def engine_config(o) -> engine.Config:
    """the engine's configuration for parsed options; NeedSites only when the block will be written: text output and
    --pretty (internal/appcore/writer_factories.go:36-38)"""
    return pipeline.engine_config(o, **_bounds(o))


def _bounds(o) -> dict:
    return dict(MinLen=o.min_length, MaxLen=o.max_length, HitCap=o.hit_cap, Circular=o.circular,
                NeedSites=pipeline.want_pretty(o))


def run(argv: Optional[Sequence[str]] = None, stdout=None, stderr=None) -> int:
    """app.RunContext -- internal/app/app.go:23-114 (scan-relevant part)."""
    stdout = stdout or sys.stdout
    stderr = stderr or sys.stderr
    o = build_parser().parse_args(argv)
    seq_files = list(o.sequences) + list(o.fasta)
    try:
        if o.primers:
            pairs = load_tsv(o.primers)
        else:
            if not o.forward or not o.reverse:
                print("error: --forward and --reverse (or --primers) are required", file=stderr)
                return 2
            pairs = [primer.Pair("manual", primer.Validate(o.forward), primer.Validate(o.reverse),
                                 o.min_length, o.max_length)]              # app.go:98
        if o.self_:
            pairs = primer.AddSelfPairsUnique(pairs) if o.multiplex else primer.AddSelfPairs(pairs)
    except (ValueError, OSError) as e:
        print(f"error: {e}", file=stderr)
        return 2
    if not seq_files:
        print("error: no FASTA input", file=stderr)
        return 2
    need_seq = o.products or o.output == "fasta"
    if o.probe and need_seq:
        print("error: --probe does not support --products or --output fasta", file=stderr)
        return 2
    eng = pipeline.new_engine(o, **_bounds(o))
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    max_primer_len = max((max(len(p.Forward), len(p.Reverse)) for p in pairs), default=0)
    chunk, overlap, warns = validate_chunking(o.circular, o.chunk_size, o.max_length, max_primer_len)
    for w in warns:
        print(f"warning: {w}", file=stderr)

    def visit(b: pipeline.Batch) -> list:                               # (product, (probe hit, site) or None, seq)
        seqs = [_text(a) for a in b.amplicons()] if need_seq else [""] * len(b.products)
        if not o.probe:
            return [(p, None, sq) for p, sq in zip(b.products, seqs)]
        out = []
        for i, h in enumerate(b.probe_hits(o.probe, o.probe_max_mm)):
            if h.found or not o.require_probe:                          # internal/visitors/probe.go:20-22
                site = b.probe_site(i, h.pos, len(primer.Normalize(o.probe))) if h.found else ""
                out.append((b.products[i], (h, site), seqs[i]))
        return out

    # the collector sees every product in the reference, chunked or not (ids.go quirk included)
    rows = pipeline.scan_files(seq_files, eng, cp, sc, chunk, overlap, Collector(o.dedup_cap), visit, stderr)
    if o.sort:
        rows.sort(key=lambda t: product_sort_key(t[0], t[1]))
    if o.output == "jsonl" and not o.probe:
        for path, p, _, sq in rows:
            print(format_jsonl(path, p, sq if o.products else ""), file=stdout)
    elif o.output == "fasta":
        for rec in fasta_records([(path, p, sq) for path, p, _, sq in rows], o.sort):
            print(rec, file=stdout)
    else:
        if not o.no_header:
            print(TSV_HEADER_PROBE if o.probe else TSV_HEADER, file=stdout)
        show = pipeline.want_pretty(o)
        for path, p, ph, _ in rows:
            line = format_row(path, p)
            block = pretty.render_product(p) if show else ""           # internal/output/text.go:21-30
            if o.probe:                                                  # probeoutput/text.go:11-28
                h, site = ph
                line += "\t" + "\t".join([o.probe_name, o.probe.upper(), "true" if h.found else "false",
                                          chr(h.strand) if h.found else "", str(h.pos) if h.found else "",
                                          str(h.mm) if h.found else "", site])
                if show:                                                 # probeoutput/pretty.go: the row's own fields
                    block = pretty.render_annotated(p, pretty.ProbeAnnotation(
                        Name=o.probe_name, Seq=o.probe.upper(), Found=bool(h.found), Strand=chr(h.strand) if h.found else "",
                        Pos=h.pos if h.found else 0, MM=h.mm if h.found else 0, Site=site))
            print(line, file=stdout)
            pipeline.write_text(stdout, block)
    return pipeline.exit_code(o, rows)


if __name__ == "__main__":
    sys.exit(run())
