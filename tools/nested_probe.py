"""Nested PCR on a large resident genome: the outer scan, then the batched inner scan of every outer amplicon
(ipcr_nested_products), and the `ipcr-nested` CLI against the plain `ipcr` CLI on the same FASTA file.

    python tools/nested_probe.py [--gbases 1] [--amplicons 100000] [--reps 3] [--cli] [--out profiles/r07_nested.json]

The genome is random ACGT (10 records) with --amplicons outer products of 300-1500 bp planted, about half of them
holding an inner product.  Host clock around each call after a device synchronise: the Python calls (ScanGenome,
NestedProducts, which build one object per product) and the bare ipcr_nested_products call; the inner scratch's filter_ms
and total_ms come from its scan statistics.  For the kernels alone run it without --cli under
`rocprofv3 --kernel-trace --stats -- python tools/nested_probe.py --reps 1`."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT_F = "ACGTTGCATGCAAGCTTAGC"
OUT_R = "GGCCTTAAGGCCATATCGTA"
IN_F = "TTGACCGATTACAGGT"
IN_R = "CCGGTTAACGGATTCA"


def rc(s: str) -> str:
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def make_records(gbases: float, amplicons: int, seed: int = 7):
    rng = np.random.default_rng(seed)
    nrec = 10
    rec_len = int(gbases * 1e9) // nrec
    lut = np.frombuffer(b"ACGT", np.uint8)
    recs = []
    per = amplicons // nrec
    of, orr, inf, inr = (np.frombuffer(s.encode(), np.uint8) for s in (OUT_F, rc(OUT_R), IN_F, rc(IN_R)))
    for r in range(nrec):
        s = lut[rng.integers(0, 4, rec_len, dtype=np.uint8)]
        slot = rec_len // per
        for k in range(per):
            a = k * slot + 100
            ln = int(rng.integers(300, 1501))
            s[a:a + 20] = of
            s[a + ln - 20:a + ln] = orr
            if k % 2 == 0:                                        # about half hold an inner product
                b = a + 30 + int(rng.integers(0, 40))
                iln = int(rng.integers(100, ln - 120))
                s[b:b + 16] = inf
                s[b + iln - 16:b + iln] = inr
        recs.append(s)
    return recs


def write_fasta(path, recs):
    with open(path, "wb") as fh:
        for r, s in enumerate(recs):
            fh.write(b">r%d\n" % r)
            n = len(s) // 80 * 80                                  # 80-base lines
            lines = np.concatenate([s[:n].reshape(-1, 80), np.full((n // 80, 1), 10, np.uint8)], axis=1)
            fh.write(lines.tobytes())
            if n < len(s):
                fh.write(s[n:].tobytes() + b"\n")


def timed_cli(module, args):
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-m", module, *args], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(f"{module} exited {p.returncode}: {p.stderr.decode()[-2000:]}")
    return dt, p.stdout.count(b"\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--amplicons", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cli", action="store_true", help="also time the ipcr-nested and ipcr CLIs end to end")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from ipcr_amd import _lib, engine, nested, primer
    t0 = time.perf_counter()
    recs = make_records(a.gbases, a.amplicons)
    gen_s = time.perf_counter() - t0
    g = engine.Genome(sum(len(s) for s in recs) + len(recs) * 8192, len(recs))
    for r, s in enumerate(recs):
        g.add_record("r%d" % r, s.tobytes())
    ocfg = engine.Config(MaxMM=0, TerminalWindow=0, MaxLen=2000, HitCap=10000, SeedLen=12)
    oeng = engine.New(ocfg)
    cpo = oeng.CompilePanel(primer.AddSelfPairs([primer.Pair("outer", OUT_F, OUT_R, 0, 2000)]))
    sco = oeng.NewSimulationScratch(cpo)
    ieng = engine.New(engine.Config(MaxMM=0, TerminalWindow=0, SeedLen=12))  # app.go:154-165: no bounds, no cap
    cpi = ieng.CompilePanel(primer.AddSelfPairs([primer.Pair("inner", IN_F, IN_R)]))
    sci = ieng.NewSimulationScratch(cpi)
    prods = oeng.ScanGenome(g, cpo, sco)                             # warm-up: kernels built, buffers grown
    nested.NestedProducts(sco, prods, g, cpi, sci)
    runs = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prods = oeng.ScanGenome(g, cpo, sco)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = nested.NestedProducts(sco, prods, g, cpi, sci)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        st = sci.stats()
        # the library calls alone, no Python object per product: the outer scan + join, then ipcr_nested_products
        n = oeng.ScanGenomeCount(g, cpo, sco)
        hits = (_lib.NestedHit * n)()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        _lib.check(_lib.lib().ipcr_nested_products(sco._h, g._h, cpi._h, sci._h, hits, n))
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        runs.append({"outer_scan_ms": (t1 - t0) * 1e3, "nested_products_ms": (t2 - t1) * 1e3,
                     "ipcr_nested_products_call_ms": (t4 - t3) * 1e3,
                     "inner_filter_ms": st.filter_ms, "inner_join_ms": st.join_ms, "inner_total_ms": st.total_ms,
                     "outer_products": len(prods), "inner_found": sum(r.InnerFound for r in res),
                     "amplicon_bases": int(sum((p.End - p.Start) for p in prods))})
    out = {"gbases": a.gbases, "planted_amplicons": a.amplicons, "reps": runs,
           "median_nested_products_ms": float(np.median([r["nested_products_ms"] for r in runs])),
           "median_outer_scan_ms": float(np.median([r["outer_scan_ms"] for r in runs])),
           "median_ipcr_nested_products_call_ms": float(np.median([r["ipcr_nested_products_call_ms"] for r in runs])),
           "genome_generate_s": gen_s, "device": torch.cuda.get_device_name(0)}
    g.close()
    for x in (sco, sci):
        x.close()
    if a.cli:
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "g.fa")
            write_fasta(fa, recs)
            common = ["-f", OUT_F, "-r", OUT_R, "--terminal-window", "0", "--max-length", "2000"]
            cli = {}
            for name, module, args in (("ipcr_text", "ipcr_amd.cli", common + [fa]),
                                       ("nested_text", "ipcr_amd.nested_cli", common + ["-F", IN_F, "-R", IN_R, fa]),
                                       ("nested_jsonl", "ipcr_amd.nested_cli", common + ["-F", IN_F, "-R", IN_R, "-o", "jsonl", fa])):
                cli[name] = [timed_cli(module, args) for _ in range(a.reps)]
            out["cli"] = {k: {"wall_s": [t for t, _ in v], "median_wall_s": float(np.median([t for t, _ in v])),
                              "lines": v[0][1]} for k, v in cli.items()}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
