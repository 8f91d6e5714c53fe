"""Minimal `ipcr-nested` driver over the HIP engine: internal/nestedapp/app.go:103-165 with the flags of
internal/nestedcli/options.go:63-118 and the common flags of `ipcr_amd.cli`.

Every outer product's amplicon is scanned with the inner panel on the device in one batch (ipcr_amd.nested); the
best inner product follows internal/visitors/nested.go:35-51.  The data paths are those of `ipcr_amd.pipeline`: NestedProducts
over a resident genome (whole records or `--chunk-size`), NestedScratchProducts over a streamed chunk.  Output: text (nestedoutput/text.go), jsonl and json (api.NestedProductV1, pkg/api/nested_v1.go);
`seq` is the outer amplicon's exact bytes, as NestedWriterFactory.NeedSeq() always asks for them.  --pretty (text) writes the
plain alignment block of the OUTER product under its row (nestedoutput/pretty.go:7-9).

    python -m ipcr_amd.nested_cli --outer-primers O.tsv --inner-primers I.tsv --output jsonl --sort g.fa
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import Optional, Sequence

from . import nested, pipeline, pretty, primer
from .cli import Collector, _text, go_json_escape, load_tsv, product_sort_key, validate_chunking

TSV_HEADER_NESTED = ("source_file\tsequence_id\touter_experiment_id\touter_start\touter_end\touter_length\touter_type\t"
                     "inner_experiment_id\tinner_found\tinner_start\tinner_end\tinner_length\tinner_type\tinner_fwd_mm"
                     "\tinner_rev_mm")                                  # internal/nestedoutput/types.go

FORMATS = ("text", "json", "jsonl", "fasta")                            # clibase.Validate accepts these four
NESTED_FORMATS = ("text", "json", "jsonl")                              # writers.WriteNested has a writer for these


class UsageError(ValueError):
    pass


def format_row(source_file: str, np: nested.NestedProduct) -> str:
    """nestedoutput.writeRowTSV -- internal/nestedoutput/text.go:9-30: the inner fields are empty only when no inner
    product was found, zeros are printed otherwise"""
    p = np.Product
    f = np.InnerFound
    inner = [str(np.InnerStart), str(np.InnerEnd), str(np.InnerLength), np.InnerType, str(np.InnerFwdMM),
             str(np.InnerRevMM)] if f else [""] * 6
    return "\t".join([source_file, p.SequenceID, p.ExperimentID, str(p.Start), str(p.End), str(p.Length), p.Type,
                      np.InnerPairID, "true" if f else "false", *inner])


def api_record(source_file: str, np: nested.NestedProduct, seq: str) -> dict:
    """api.NestedProductV1 (pkg/api/nested_v1.go) as encoding/json orders and omits its fields: the struct's order,
    `omitempty` fields left out when zero or empty, inner_found always present (score: thermo builds only)"""
    p = np.Product
    d = {"experiment_id": p.ExperimentID, "sequence_id": p.SequenceID, "start": p.Start, "end": p.End,
         "length": p.Length, "type": p.Type}
    for key, v in (("fwd_mm", p.FwdMM), ("rev_mm", p.RevMM), ("fwd_mm_i", list(p.FwdMismatchIdx)),
                   ("rev_mm_i", list(p.RevMismatchIdx)), ("seq", seq), ("source_file", source_file)):
        if v:
            d[key] = v
    d["inner_found"] = np.InnerFound
    for key, v in (("inner_experiment_id", np.InnerPairID), ("inner_start", np.InnerStart), ("inner_end", np.InnerEnd),
                   ("inner_length", np.InnerLength), ("inner_type", np.InnerType), ("inner_fwd_mm", np.InnerFwdMM),
                   ("inner_rev_mm", np.InnerRevMM)):
        if v:
            d[key] = v
    return d


def format_jsonl(source_file: str, np: nested.NestedProduct, seq: str) -> str:
    """one line of the JSONL writer (internal/writers/nested_jsonl.go: json.Encoder.Encode, compact)"""
    return go_json_escape(json.dumps(api_record(source_file, np, seq), separators=(",", ":"), ensure_ascii=False))


def format_json(rows) -> str:
    """the JSON array of (source_file, NestedProduct, seq) rows: jsonutil.EncodePretty, two-space indent, final newline"""
    return go_json_escape(json.dumps([api_record(path, np, sq) for path, np, sq in rows], indent=2,
                                     ensure_ascii=False)) + "\n"


def sort_rows(rows) -> list:
    """sort.SliceStable by common.LessProduct over the outer product (internal/writers/nested.go); Seq is its last key"""
    return sorted(rows, key=lambda t: product_sort_key(t[0], t[1].Product) + (t[2],))


def effective_max_len(global_max: int, pairs: Sequence[primer.Pair]) -> int:
    """appcore.effectiveMaxProductLen -- internal/appcore/core.go: the largest per-pair bound, 0 (unbounded) when a pair
    without one meets an unbounded --max-length"""
    eff, unbounded = global_max, False
    for p in pairs:
        if p.MaxProduct > 0:
            eff = max(eff, p.MaxProduct)
        elif global_max <= 0:
            unbounded = True
    return 0 if unbounded else eff


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="ipcr-nested-hip", add_help=True)
    ap.add_argument("--primers", "--outer-primers", "-p", dest="primers", default="")
    ap.add_argument("--forward", "-f", default="")
    ap.add_argument("--reverse", "-r", default="")
    ap.add_argument("--inner-primers", "-P", default="")
    ap.add_argument("--inner-forward", "-F", default="")
    ap.add_argument("--inner-reverse", "-R", default="")
    ap.add_argument("--require-inner", action="store_true", help="only keep outer amplicons that contain an inner product")
    pipeline.add_common_flags(ap, dict(help="text | json | jsonl"), "scan rolling chunks (0 = whole records resident)")
    return ap


def _inline_pair(what: str, path: str, fwd: str, rev: str):
    """the primer rules of clibase.Validate (outer) and nestedcli.ParseArgs (inner): (validated fwd, rev) or None when
    the TSV file is used"""
    flag = "--" if what == "outer" else "--inner-"
    files = "--primers" if what == "outer" else "--inner-primers"
    inline = bool(fwd or rev)
    if path and inline:
        raise UsageError(f"{files} conflicts with {flag}forward/{flag}reverse")
    if inline and not (fwd and rev):
        raise UsageError(f"{flag}forward and {flag}reverse must be supplied together")
    if not path and not inline:
        raise UsageError(f"provide {files} or {flag}forward/{flag}reverse")
    if not inline:
        return None
    out = []
    for name, v in (("forward", fwd), ("reverse", rev)):
        try:
            out.append(primer.Validate(v))
        except ValueError as e:
            raise UsageError(f"{flag}{name}: {e}")
    return out


def parse(argv: Optional[Sequence[str]]):
    """options + (outer pairs, inner pairs); UsageError for everything nestedcli.ParseArgs / clibase.Validate refuse"""
    o = build_parser().parse_args(argv)
    o.seq_files = list(o.sequences) + list(o.fasta)
    outer_inline = _inline_pair("outer", o.primers, o.forward, o.reverse)
    if not o.seq_files:
        raise UsageError("at least one sequence file is required")
    for name, v in (("--chunk-size", o.chunk_size), ("--hit-cap", o.hit_cap), ("--dedup-cap", o.dedup_cap)):
        if v < 0:
            raise UsageError(f"{name} must be >= 0")
    if o.output not in FORMATS:
        raise UsageError(f"invalid --output {json.dumps(o.output)}")
    if o.terminal_window < -1:
        raise UsageError("--terminal-window must be >= -1")
    if not 0 <= o.no_match_exit_code <= 255:
        raise UsageError("--no-match-exit-code must be between 0 and 255")
    inner_inline = _inline_pair("inner", o.inner_primers, o.inner_forward, o.inner_reverse)
    try:                                                                # app.go:103-139
        outer = load_tsv(o.primers) if outer_inline is None else \
            [primer.Pair("outer", outer_inline[0], outer_inline[1], o.min_length, o.max_length)]
        inner = load_tsv(o.inner_primers) if inner_inline is None else [primer.Pair("inner", *inner_inline)]
    except (ValueError, OSError) as e:
        raise UsageError(str(e))
    if o.self_:
        outer, inner = primer.AddSelfPairs(outer), primer.AddSelfPairs(inner)
    return o, outer, inner


def run(argv: Optional[Sequence[str]] = None, stdout=None, stderr=None) -> int:
    """nestedapp.RunContext + appcore.Run (internal/appcore/core.go) for the scan path."""
    stdout = stdout or sys.stdout
    stderr = stderr or sys.stderr
    try:
        o, outer_pairs, inner_pairs = parse(argv)
    except SystemExit as e:                                             # argparse: -h (0) or a malformed flag (2)
        return int(e.code or 0)
    except UsageError as e:
        print(f"error: {e}", file=stderr)
        return 2
    max_primer_len = max((max(len(p.Forward), len(p.Reverse)) for p in outer_pairs), default=0)
    eff_max = effective_max_len(o.max_length, outer_pairs)
    if 0 < eff_max < max_primer_len:
        print(f"error: effective maximum product length ({eff_max}) is smaller than the longest primer length "
              f"({max_primer_len})", file=stderr)
        return 2
    if o.min_length > 0 and o.max_length > 0 and o.min_length > o.max_length:
        print(f"error: --min-length ({o.min_length}) exceeds --max-length ({o.max_length})", file=stderr)
        return 2
    if o.output not in NESTED_FORMATS:                                  # writers.WriteNested (registry.go:45-51)
        print(f"unknown nested format {json.dumps(o.output)} (no writer registered)", file=stderr)
        return 3
    chunk, overlap, warns = validate_chunking(o.circular, o.chunk_size, eff_max, max_primer_len)
    for w in warns:
        print(f"warning: {w}", file=stderr)
    eng = pipeline.new_engine(o, MinLen=o.min_length, MaxLen=o.max_length, HitCap=o.hit_cap, Circular=o.circular,
                              NeedSites=pipeline.want_pretty(o))
    cp = eng.CompilePanel(outer_pairs)
    sc = eng.NewSimulationScratch(cp)
    ieng = pipeline.new_engine(o)       # the inner engine (app.go:154-165): linear amplicons, no length bounds, no hit cap
    cpi = ieng.CompilePanel(inner_pairs)
    sci = ieng.NewSimulationScratch(cpi)

    def visit(b: pipeline.Batch) -> list:                               # (outer product, NestedProduct, seq)
        return [(np.Product, np, _text(a)) for np, a in zip(b.nested(cpi, sci), b.amplicons())]

    # the collector, then visitors.Nested.Visit; rows: (source_file, NestedProduct, seq)
    rows = [(path, np, sq) for path, _, np, sq in
            pipeline.scan_files(o.seq_files, eng, cp, sc, chunk, overlap, Collector(o.dedup_cap), visit, stderr)
            if np.InnerFound or not o.require_inner]
    if o.sort:
        rows = sort_rows(rows)
    if o.output == "json":
        stdout.write(format_json(rows))
    elif o.output == "jsonl":
        for path, np, sq in rows:
            print(format_jsonl(path, np, sq), file=stdout)
    else:
        if not o.no_header:
            print(TSV_HEADER_NESTED, file=stdout)
        for path, np, _ in rows:
            print(format_row(path, np), file=stdout)
            if pipeline.want_pretty(o):
                pipeline.write_text(stdout, pretty.render_product(np.Product))
    return pipeline.exit_code(o, rows)


if __name__ == "__main__":
    sys.exit(run())
