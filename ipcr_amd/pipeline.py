"""One input file -> batches of products plus access to their amplicons: what `ipcr_amd.cli` and `ipcr_amd.nested_cli`
share of internal/pipeline (pipeline.go:60-182) and internal/clibase (common.go:61-110).

Three data paths, chosen here and nowhere else: whole records resident (ScanGenome), `--chunk-size` over a resident genome
(ScanGenomeChunked: one sweep, window-local products) and streamed chunks (fasta.StreamChunks +
SimulateCompiledWithScratch: IPCR_CLI_STREAM_CHUNKS=1, and the fall-back of the second path).  A driver supplies
`visit(batch) -> [(product, ...)]`; what it returns reaches the collector only when the whole visit succeeded."""
from __future__ import annotations

import argparse
import os
from typing import Callable, List, Sequence

from . import _lib, engine, fasta, nested


def add_common_flags(ap: argparse.ArgumentParser, output: dict, chunk_size_help: str) -> None:
    """the flags every driver takes, names and defaults of internal/clibase/common.go:61-110; `output` and the help of
    --chunk-size differ per driver"""
    ap.add_argument("--sequences", "-s", action="append", default=[])
    ap.add_argument("--mismatches", "-m", type=int, default=0)
    ap.add_argument("--min-length", type=int, default=0)
    ap.add_argument("--max-length", type=int, default=2000)
    ap.add_argument("--hit-cap", type=int, default=10000)
    ap.add_argument("--terminal-window", type=int, default=3)
    ap.add_argument("--self", dest="self_", action=argparse.BooleanOptionalAction, default=True)
    ap.add_argument("--seed-length", type=int, default=12)
    ap.add_argument("--circular", "-c", action="store_true")
    ap.add_argument("--sort", action="store_true")
    ap.add_argument("--output", "-o", default="text", **output)
    ap.add_argument("--no-header", action="store_true")
    ap.add_argument("--pretty", action="store_true", help="text output: the alignment block under every row")
    ap.add_argument("--no-match-exit-code", type=int, default=0)
    ap.add_argument("--chunk-size", type=int, default=0, help=chunk_size_help)
    ap.add_argument("--dedup-cap", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("fasta", nargs="*")


def want_pretty(o) -> bool:
    """the block is written, and the engine asked for sites, only by the text writer (appcore/writer_factories.go:36-38);
    every other format accepts the flag and ignores it"""
    return bool(o.pretty) and o.output == "text"


def new_engine(o, **bounds) -> engine.Engine:
    """the engine of the common flags on --device; `bounds`: MinLen / MaxLen / HitCap / Circular / NeedSites, which the
    inner engine of ipcr-nested leaves at zero"""
    _lib.check(_lib.lib().ipcr_set_device(o.device))
    return engine.New(engine_config(o, **bounds))


def engine_config(o, **bounds) -> engine.Config:
    tw = o.terminal_window if o.terminal_window >= 1 else 0            # runutil.EffectiveTerminalWindow
    return engine.Config(MaxMM=o.mismatches, TerminalWindow=tw, SeedLen=o.seed_length, **bounds)


def write_text(stdout, text: str) -> None:
    """`text` to the driver's stdout handle as UTF-8 (the pretty block holds a non-ASCII glyph): a text handle that cannot
    encode it and has a byte buffer underneath gets the bytes, every other handle the string"""
    if not text:
        return
    enc = (getattr(stdout, "encoding", None) or "utf-8").lower().replace("-", "").replace("_", "")
    buf = getattr(stdout, "buffer", None)
    if enc != "utf8" and buf is not None:
        stdout.flush()
        buf.write(text.encode("utf-8"))
        buf.flush()
    else:
        stdout.write(text)


def exit_code(o, rows) -> int:
    return o.no_match_exit_code if not rows else 0


def _cut(seq: bytes, start: int, end: int) -> bytes:
    return seq[start:end] if start <= end else seq[start:] + seq[:end]  # start > end: a product across the origin


class Batch:
    """The products of one scan and where their amplicons lie: in a resident genome (`windows`: the rolling windows
    the products are local to, None for whole records) or in the chunk the scratch holds."""

    def __init__(self, products, sc, genome=None, windows=None, chunk: bytes = b"", path: str = ""):
        self.products, self.sc, self.genome, self.chunk, self.path = products, sc, genome, chunk, path
        if genome is None:
            self.windows = None
        elif windows is None:
            self.windows = [(p.Record, p.Start, p.End) for p in products]
        else:                                                           # window-local -> record coordinates
            self.windows = [(windows[p.Record].record, windows[p.Record].start + p.Start,
                             windows[p.Record].start + p.End) for p in products]

    def amplicons(self) -> List[bytes]:
        """exact bytes of every product, as loaded"""
        if self.genome is None:
            return [_cut(self.chunk, p.Start, p.End) for p in self.products]
        try:
            return self.genome.read_windows(self.windows)
        except _lib.IpcrError as e:
            if e.status != _lib.ERR_UNSUPPORTED:
                raise
        recs = self._host_records()
        return [_cut(recs[r], a, b) for r, a, b in self.windows]

    def _host_records(self) -> dict:
        """the genome keeps no exception runs: the records the products lie in, streamed whole on the host"""
        wanted, recs = {r for r, _, _ in self.windows}, {}
        for i, rec in enumerate(fasta.StreamChunks(self.path, 0, 0)):
            if i in wanted:
                recs[i] = rec.Seq
        return recs

    def sites(self) -> List[tuple]:
        """(FwdSite, RevSite) of every product (core/engine/engine.go:177-185): read and reverse-complemented on the
        device for a resident genome (one call), sliced from the chunk in hand otherwise"""
        if self.genome is None:
            return [engine.host_sites(self.chunk, p.Start, p.End, len(p.FwdPrimer), len(p.RevPrimer)) for p in self.products]
        try:
            return self.sc.product_sites(self.genome)
        except _lib.IpcrError as e:
            if e.status != _lib.ERR_UNSUPPORTED:
                raise
        recs = self._host_records()
        return [engine.host_sites(recs[r], a, b, len(p.FwdPrimer), len(p.RevPrimer))
                for p, (r, a, b) in zip(self.products, self.windows)]

    def thermo_scores(self, denoms=None) -> List[float]:
        """the legacy-heuristic Score of every product (internal/thermovisitors/score.go:1522-1552), computed on the
        device from the tiles the products were found in: the resident genome, or the chunk the scratch holds.  `denoms`:
        thermo.panel_denoms (--denom auto), None for 200.0."""
        return self.sc.thermo_scores(self.genome, denoms)

    def thermo_nn_scores(self, base, anneal_c: float, details: bool = False):
        """the nn-duplex-v1 Score of every product (score.go:637-690), computed on the device from the same tiles.  `base`:
        thermo.panel_nn_base; details: -> (scores, ends) as engine.SimulationScratch.thermo_nn_scores"""
        return self.sc.thermo_nn_scores(self.genome, base, anneal_c, details)

    def probe_hits(self, probe: str, max_mm: int):
        """ipcr-probe keeps --chunk-size (internal/probeapp/app.go:108): every product is annotated from its own
        amplicon, rescanned from the tiles it was found in (pipeline.go:80-89 slices Product.Seq chunk-locally too)"""
        return self.sc.probe_products(probe, max_mm, self.genome)

    def probe_site(self, i: int, pos: int, n: int) -> str:
        """`n` bases at `pos` of product i's amplicon, upper case.  The two sources differ: a resident genome is read
        back from its tiles, where every byte outside ACGTacgt decodes as N; a chunk gives its own bytes, IUPAC codes
        kept.  Each path keeps the source it always had."""
        if self.genome is None:
            amp = _cut(self.chunk, self.products[i].Start, self.products[i].End)
        else:
            g, (r, a, b) = self.genome, self.windows[i]
            amp = g.read(r, a, b - a) if a <= b else g.read(r, a, g.record_len(r) - a) + g.read(r, 0, b)
        return amp.upper()[pos:pos + n].decode()

    def nested(self, inner: engine.CompiledPanel, inner_scratch: engine.SimulationScratch):
        """the best inner product of every amplicon (internal/visitors/nested.go:35-51), scanned on the device"""
        if self.genome is None:
            return nested.NestedScratchProducts(self.sc, self.products, inner, inner_scratch)
        return nested.NestedProducts(self.sc, self.products, self.genome, inner, inner_scratch)


def scan_files(paths: Sequence[str], eng: engine.Engine, cp: engine.CompiledPanel, sc: engine.SimulationScratch,
               chunk: int, overlap: int, collector, visit: Callable[[Batch], list], stderr) -> list:
    """Every file through its data path; rows (path, product, ...) of what `visit` returned and the collector kept, in
    emission order.  A file that fails is reported and the next one scanned (pipeline.go:174-182)."""
    rows = []

    def keep(path: str, batch: Batch) -> None:
        if batch.products:
            if cp.Cfg.NeedSites and batch.genome is not None:           # (a streamed chunk's products have theirs)
                for p, (fwd, rev) in zip(batch.products, batch.sites()):
                    p.FwdSite, p.RevSite = fwd, rev
            for p, *rest in visit(batch):                               # (raises before the first row is kept)
                if collector.add(path, p) is not None:
                    rows.append((path, p, *rest))

    for path in paths:
        try:
            if not (chunk and os.environ.get("IPCR_CLI_STREAM_CHUNKS")):
                size = os.path.getsize(path) if path != "-" and os.path.exists(path) else (1 << 28)
                g = engine.Genome(max(size * (8 if path.endswith(".gz") else 1), 1 << 20), max_records=1 << 16)
                try:
                    g.add_fasta(path)
                    # whole records, or --chunk-size: one sweep, every rolling window joined on its own
                    prods = eng.ScanGenomeChunked(g, cp, sc, chunk, overlap, sites=False) if chunk else \
                        eng.ScanGenome(g, cp, sc, sites=False)
                    keep(path, Batch(prods, sc, g, sc.chunk_windows() if chunk else None, path=path))
                    continue
                except _lib.IpcrError as e:                             # (a capped scan that ran in segments: stream the chunks)
                    if not (chunk and e.status == _lib.ERR_UNSUPPORTED):
                        raise
                finally:
                    g.close()
            # the reference's data path: every rolling chunk goes through the engine on its own (ForEachCompiledProduct
            # = ipcr_scan_chunk), the collector restores record coordinates
            for rec in fasta.StreamChunks(path, chunk, overlap):
                keep(path, Batch(eng.SimulateCompiledWithScratch(rec.ID, rec.Seq, cp, sc), sc, chunk=rec.Seq))
        except _lib.IpcrError as e:
            print(f"error: {e}", file=stderr)
    return rows
