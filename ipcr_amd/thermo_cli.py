"""Minimal `ipcr-thermo` driver over the HIP engine, `--thermo-model legacy-heuristic` only: internal/thermoapp/app.go with
the flags and defaults of internal/thermocli/options.go and the common flags of `ipcr_amd.cli`.

Every product's Score is computed on the device from the tiles it was found in (ipcr_thermo_legacy_products /
ipcr_thermo_legacy_scratch_products, one call per batch); the host computes one denominator per primer for `--denom auto`
(ipcr_amd.thermo).  Output is always sorted: by score, higher first, unless `--rank coord`.  text carries the trailing `score`
column, jsonl `seq` and `score`, fasta the amplicons.  The data paths are those of `ipcr_amd.pipeline`.

Not built, and refused by name with exit 2 instead of printing other numbers: the NN models (`nn-duplex-v1`, and
`nn-structure-v1`, the reference's default -- so `--thermo-model legacy-heuristic` must be given), `--single-stranded`,
`--probe`, `--thermo-details`, `--pretty` and `--output json`.

    python -m ipcr_amd.thermo_cli --thermo-model legacy-heuristic -f AAGTAC -r GGTACC -m 1 --seed-length 3 ref.fa
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import List, Optional, Sequence

from . import pipeline, primer, thermo
from .cli import (TSV_HEADER, Collector, _text, fasta_records, format_row, go_json_escape, load_tsv, product_sort_key,
                  validate_chunking)
from .nested_cli import UsageError, effective_max_len

FORMATS = ("text", "json", "jsonl", "fasta")                            # clibase.Validate accepts these four
_BOOL_FLAGS = {"--self": "--no-self", "--circular": None, "-c": None, "--sort": None, "--no-header": None, "--pretty": None,
               "--products": None, "--allow-indel": None, "--single-stranded": None, "--thermo-details": None,
               "--quiet": None, "-q": None, "--probe-thermo": "--no-probe-thermo", "--struct-hairpin": "--no-struct-hairpin",
               "--struct-dimer": "--no-struct-dimer"}


def _go_bools(argv: Sequence[str]) -> List[str]:
    """Go's flag package writes a boolean as `--self=false`; argparse wants `--no-self`"""
    out = []
    for a in argv:
        name, eq, val = a.partition("=")
        if eq and name in _BOOL_FLAGS and val.lower() in ("true", "false", "1", "0", "t", "f"):
            if val.lower() in ("true", "1", "t"):
                out.append(name)
            elif _BOOL_FLAGS[name]:
                out.append(_BOOL_FLAGS[name])
        else:
            out.append(a)
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="ipcr-thermo-hip", add_help=True)
    ap.add_argument("--primers", "-p", default="")
    ap.add_argument("--forward", "-f", default="")
    ap.add_argument("--reverse", "-r", default="")
    pipeline.add_common_flags(ap, dict(help="text | jsonl | fasta"), "scan rolling chunks (0 = whole records resident)")
    ap.add_argument("--products", action="store_true", help="accepted: ipcr-thermo always carries the sequences")
    ap.add_argument("--quiet", "-q", action="store_true")
    ap.add_argument("--threads", "-t", type=int, default=0, help="accepted: the scan runs on the device")
    ap.add_argument("--oligo", action="append", default=[], help="oligo (ID:SEQ or SEQ); repeatable")
    ap.add_argument("--oligos", default="", help="oligo TSV: id seq")
    ap.add_argument("--anneal-temp", type=float, default=60.0)
    ap.add_argument("--na", default="50mM")
    ap.add_argument("--mg", default="3mM")
    ap.add_argument("--dntp", default="0mM")
    ap.add_argument("--primer-conc", default="250nM")
    ap.add_argument("--salt-model", default=thermo.SALT_MONOVALENT, help=thermo.KNOWN_SALT_MODELS)
    ap.add_argument("--allow-indel", action="store_true", help="accepted: cannot change a legacy-heuristic score")
    ap.add_argument("--single-stranded", action="store_true", help="not built (needs the hairpin model)")
    ap.add_argument("--thermo-model", default="", help=f"{thermo.LEGACY_HEURISTIC} (required; the NN models are not built)")
    ap.add_argument("--iupac-thermo-policy", default="worst", help="NN models only")
    ap.add_argument("--iupac-thermo-max-expansions", type=int, default=256, help="NN models only")
    ap.add_argument("--denom", default="fixed", help="fixed (D = 200) | auto (from each primer's own Tm)")
    ap.add_argument("--probe", default="", help="not built")
    ap.add_argument("--probe-name", default="probe")
    ap.add_argument("--probe-max-mm", type=int, default=0)
    ap.add_argument("--probe-thermo", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--probe-score-mode", default="gate")
    ap.add_argument("--probe-min-margin", type=float, default=0.0)
    ap.add_argument("--probe-weight", type=float, default=1.0)
    ap.add_argument("--rank", default="score", help="score | coord")
    ap.add_argument("--thermo-details", action="store_true", help="not built (NN component columns)")
    # the thermo extensions act in the NN models only (score.go:1506-1519: the legacy model returns before them)
    ap.add_argument("--score-profile", default="binding")
    ap.add_argument("--ext-alpha", type=float, default=0.45)
    ap.add_argument("--length-knee-bp", type=int, default=550)
    ap.add_argument("--length-steep", type=float, default=0.003)
    ap.add_argument("--length-max-pen", type=float, default=10.0)
    ap.add_argument("--band-mass-weight", type=float, default=15.0)
    ap.add_argument("--struct-hairpin", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--struct-dimer", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--struct-scale", type=float, default=1.0)
    ap.add_argument("--bind-weight", type=float, default=1.0)
    ap.add_argument("--ext-weight", type=float, default=1.0)
    return ap


def _oligo(seq: str, what: str) -> str:
    """oligo.Validate -- core/oligo/validate.go:50-61"""
    try:
        return primer.Validate(seq)
    except ValueError as e:
        raise UsageError(f"{what}: {e}")


def parse_oligo_inline(spec: str, idx: int) -> primer.Oligo:
    """parseOligoInline -- app.go:29-48: `ID:SEQ` or `SEQ` (ID O<position>)"""
    spec = spec.strip()
    if not spec:
        raise UsageError(f"empty --oligo at position {idx + 1}")
    oid, seq = "", spec
    if ":" in spec:
        oid, _, seq = spec.partition(":")
        oid, seq = oid.strip(), seq.strip()
    return primer.Oligo(oid or f"O{idx + 1}", _oligo(seq, f"--oligo {json.dumps(spec)}"))


def load_oligos_tsv(path: str) -> List[primer.Oligo]:
    """loadOligosTSV -- app.go:50-88: `seq` or `id seq` per line"""
    out: List[primer.Oligo] = []
    try:
        fh = open(path)
    except OSError as e:
        raise UsageError(str(e))
    with fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line[0] == "#":
                continue
            f = line.split()
            if len(f) == 1:
                out.append(primer.Oligo(f"O{len(out) + 1}", _oligo(f[0], f"{path}:{ln}")))
            elif len(f) == 2:
                out.append(primer.Oligo(f[0], _oligo(f[1], f"{path}:{ln}")))
            else:
                raise UsageError(f"{path}:{ln}: expected 1 or 2 columns (id seq), got {len(f)}")
    return out


def pairs_from_oligos(oligos: Sequence[primer.Oligo], min_len: int, max_len: int, include_self: bool) -> List[primer.Pair]:
    """pairsFromOligos -- app.go:90-107: every unordered pair `A+B`, then the self pairs"""
    out = [primer.Pair(f"{a.ID}+{b.ID}", a.Seq.upper(), b.Seq.upper(), min_len, max_len)
           for i, a in enumerate(oligos) for b in oligos[i + 1:]]
    if include_self:
        out += primer.SelfPairs(oligos)
    return out


def _refuse(what: str) -> UsageError:
    return UsageError(f"{what}; this build scores with --thermo-model {thermo.LEGACY_HEURISTIC} only")


def parse(argv: Optional[Sequence[str]]):
    """options + pairs + conditions; UsageError (exit 2) for what thermocli.ParseArgs / thermoapp refuse and for everything
    this build does not score.  Nothing here touches a device."""
    o = build_parser().parse_args(_go_bools(list(sys.argv[1:] if argv is None else argv)))
    o.seq_files = list(o.sequences) + list(o.fasta)
    # -- the model first: a run that would print other numbers than the reference's must not start
    model = o.thermo_model.strip().lower()
    if model == "":
        raise _refuse("--thermo-model is required: the reference's default is nn-structure-v1, which is not built")
    if model in thermo.UNBUILT_MODELS:
        raise _refuse(f"--thermo-model {model} is not built")
    if model != thermo.LEGACY_HEURISTIC:
        raise UsageError(f"unknown thermo model {json.dumps(o.thermo_model)}; expected one of: "
                         f"{' | '.join((thermo.LEGACY_HEURISTIC,) + thermo.UNBUILT_MODELS)}")
    if o.single_stranded:
        raise _refuse("--single-stranded needs the hairpin model, which is not built")
    if o.probe.strip():
        raise _refuse("--probe is not built (probe thermodynamics need the NN models)")
    if o.thermo_details:
        raise _refuse("--thermo-details is not built (its columns are NN components)")
    if o.pretty:
        raise _refuse("--pretty is not built for ipcr-thermo")
    if o.output not in FORMATS:
        raise UsageError(f"invalid --output {json.dumps(o.output)}")
    if o.output == "json":
        raise _refuse("--output json is not built (text, jsonl and fasta are)")
    # -- thermocli.ParseArgs
    inline = bool(o.forward or o.reverse)
    if inline and not (o.forward and o.reverse):
        raise UsageError("--forward and --reverse must be supplied together")
    oligo_mode = bool(o.oligo or o.oligos)
    pair_mode = bool(o.primers or inline)
    if oligo_mode and pair_mode:
        raise UsageError("--oligo/--oligos cannot be combined with --primers or --forward/--reverse")
    if not oligo_mode and not pair_mode:
        raise UsageError("provide --oligo/--oligos OR --primers/--forward+--reverse")
    if o.primers and inline:
        raise UsageError("--primers conflicts with --forward/--reverse")
    if not o.seq_files:
        raise UsageError("at least one sequence file is required (positional or --sequences)")
    if o.rank.lower() not in ("coord", "score"):
        raise UsageError("--rank must be 'coord' or 'score'")
    if o.denom.lower() not in ("fixed", "auto"):
        raise UsageError("--denom must be 'fixed' or 'auto'")
    if o.score_profile.lower() not in ("binding", "pcr", "gel"):
        raise UsageError("--score-profile must be 'binding', 'pcr', or 'gel'")
    if o.iupac_thermo_policy.strip().lower() not in ("strict", "worst", "best", "mean", "enumerate"):
        raise UsageError(f"unknown --iupac-thermo-policy {json.dumps(o.iupac_thermo_policy)}")
    if o.iupac_thermo_max_expansions < 1:
        raise UsageError("--iupac-thermo-max-expansions must be >= 1")
    for name, v in (("--ext-alpha", o.ext_alpha), ("--length-knee-bp", o.length_knee_bp), ("--length-steep", o.length_steep),
                    ("--length-max-pen", o.length_max_pen), ("--band-mass-weight", o.band_mass_weight),
                    ("--chunk-size", o.chunk_size), ("--hit-cap", o.hit_cap), ("--dedup-cap", o.dedup_cap)):
        if v < 0:
            raise UsageError(f"{name} must be >= 0")
    if o.probe_score_mode.lower() not in ("annotate", "gate", "blend"):
        raise UsageError("--probe-score-mode must be 'annotate', 'gate', or 'blend'")
    if not -100 <= o.probe_min_margin <= 100:
        raise UsageError("--probe-min-margin must be within [-100,100]")
    if not 0 <= o.probe_weight <= 1:
        raise UsageError("--probe-weight must be in [0,1]")
    if o.terminal_window < -1:
        raise UsageError("--terminal-window must be >= -1")
    if not 0 <= o.no_match_exit_code <= 255:
        raise UsageError("--no-match-exit-code must be between 0 and 255")
    try:
        salt = thermo.ParseSaltModel(o.salt_model)
    except ValueError as e:
        raise UsageError(str(e))
    # -- thermoapp.RunContext: the panel (app.go:248-312)
    if oligo_mode:
        oligos = load_oligos_tsv(o.oligos) if o.oligos else []
        oligos += [parse_oligo_inline(spec, i) for i, spec in enumerate(o.oligo)]
        if not oligos:
            raise UsageError("no oligos provided")
        pairs = pairs_from_oligos(oligos, o.min_length, o.max_length, o.self_)
        if not pairs:
            raise UsageError("need ≥2 oligos for pairing (or enable --self)")
    else:
        try:
            if o.primers:
                pairs = load_tsv(o.primers)
            else:
                pairs = [primer.Pair("manual", primer.Validate(o.forward).upper(), primer.Validate(o.reverse).upper(),
                                     o.min_length, o.max_length)]
        except (ValueError, OSError) as e:
            raise UsageError(str(e))
        if o.self_:
            pairs = primer.AddSelfPairsUnique(pairs)                     # (ipcr-thermo adds each oligo's self pair once)
    return o, pairs, salt


def conditions(o, salt: str, stderr) -> thermo.Conditions:
    """the solution conditions of app.go:314-348: a value that does not parse is warned about and replaced by its default"""
    vals = []
    for flag, spec, dflt, shown in (("--na", o.na, 0.05, "50mM"), ("--mg", o.mg, 0.003, "3mM"), ("--dntp", o.dntp, 0.0, "0mM"),
                                    ("--primer-conc", o.primer_conc, 2.5e-7, "250nM")):
        try:
            vals.append(thermo.ParseConc(spec))
        except ValueError as e:
            if not o.quiet:
                print(f"WARN: bad {flag} {json.dumps(spec)}: {e} (using {shown})", file=stderr)
            vals.append(dflt)
    return thermo.Conditions(AnnealC=o.anneal_temp, NaM=vals[0], MgM=vals[1], DntpM=vals[2], PrimerTotalM=vals[3], SaltModel=salt)


def format_jsonl(source_file: str, p, seq: str) -> str:
    """api.ProductV1 (pkg/api/products_v1.go:6-25) with the thermo fields: `seq` always (the thermo writer asks for the
    sequences), `score` behind source_file and left out when it is zero of either sign (omitempty)"""
    d = {"experiment_id": p.ExperimentID, "sequence_id": p.SequenceID, "start": p.Start, "end": p.End, "length": p.Length,
         "type": p.Type}
    for key, v in (("fwd_mm", p.FwdMM), ("rev_mm", p.RevMM), ("fwd_mm_i", list(p.FwdMismatchIdx)),
                   ("rev_mm_i", list(p.RevMismatchIdx)), ("seq", seq), ("source_file", source_file)):
        if v:
            d[key] = v
    line = go_json_escape(json.dumps(d, separators=(",", ":"), ensure_ascii=False))
    if p.Score != 0:
        line = line[:-1] + ',"score":' + thermo.go_json_float(p.Score) + "}"
    return line


def sort_rows(rows, by_score: bool) -> list:
    """common.SortProductsByScore / SortProducts (internal/common/sort.go:76-99) over (source_file, product, seq) rows"""
    def key(t):
        k = product_sort_key(t[0], t[1]) + (t[2],)
        return thermo.score_rank(t[1].Score) + k if by_score else k
    return sorted(rows, key=key)


def run(argv: Optional[Sequence[str]] = None, stdout=None, stderr=None) -> int:
    """thermoapp.RunContext + appcore.Run for the scan path"""
    stdout = stdout or sys.stdout
    stderr = stderr or sys.stderr
    try:
        o, pairs, salt = parse(argv)
    except SystemExit as e:                                             # argparse: -h (0) or a malformed flag (2)
        return int(e.code or 0)
    except UsageError as e:
        print(f"error: {e}", file=stderr)
        return 2
    cond = conditions(o, salt, stderr)
    max_primer_len = max((max(len(p.Forward), len(p.Reverse)) for p in pairs), default=0)
    eff_max = effective_max_len(o.max_length, pairs)
    if 0 < eff_max < max_primer_len:
        print(f"error: effective maximum product length ({eff_max}) is smaller than the longest primer length "
              f"({max_primer_len})", file=stderr)
        return 2
    if o.min_length > 0 and o.max_length > 0 and o.min_length > o.max_length:
        print(f"error: --min-length ({o.min_length}) exceeds --max-length ({o.max_length})", file=stderr)
        return 2
    chunk, overlap, warns = validate_chunking(o.circular, o.chunk_size, eff_max, max_primer_len)
    for w in warns:
        if not o.quiet:
            print(f"warning: {w}", file=stderr)
    denoms = thermo.panel_denoms(pairs, cond if o.denom.lower() == "auto" else None)   # one D per primer, not per product
    eng = pipeline.new_engine(o, MinLen=o.min_length, MaxLen=o.max_length, HitCap=o.hit_cap, Circular=o.circular)
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    need_seq = o.output != "text"                                       # (the text writer never prints Seq)

    def visit(b: pipeline.Batch) -> list:                               # (product with its Score, seq)
        seqs = [_text(a) for a in b.amplicons()] if need_seq else [""] * len(b.products)
        for p, s in zip(b.products, b.thermo_scores(denoms)):
            p.Score = s
        return list(zip(b.products, seqs))

    rows = pipeline.scan_files(o.seq_files, eng, cp, sc, chunk, overlap, Collector(o.dedup_cap), visit, stderr)
    rows = sort_rows(rows, o.rank.lower() != "coord")                  # (the thermo writer always sorts: app.go:431-433)
    if o.output == "jsonl":
        for path, p, sq in rows:
            print(format_jsonl(path, p, sq), file=stdout)
    elif o.output == "fasta":
        for rec in fasta_records(rows, True):
            print(rec, file=stdout)
    else:
        if not o.no_header:
            print(TSV_HEADER + "\tscore", file=stdout)
        for path, p, _ in rows:
            print(format_row(path, p) + "\t" + thermo.go_g(p.Score), file=stdout)   # output/rows.go:31-35
    return pipeline.exit_code(o, rows)


if __name__ == "__main__":
    sys.exit(run())
