#!/usr/bin/env python3
"""dev tool (GPU box): FASTA load time of two builds of the library, A/B/A/B in fresh child processes -- for the exception
runs: an +N genome (ACGT with N runs, zero exception runs) and the same genome with an 'R' every ~10 kb, each
through the default loader and the device loader (IPCR_FASTA_HOSTPACK=0).

    python3 tools/fasta_load_exc_ab.py A=path/to/libipcr_hip.so B=ipcr_amd/libipcr_hip.so [--gbases 1] [--rounds 3] [--out f.json]

The children call the C ABI through ctypes directly (ipcr_genome_create / _add_fasta / _destroy), so an older build that
lacks newer symbols loads too."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

FILES = {"plus_n": "/tmp/ipcr_exc_ab_n.fa", "iupac_10kb": "/tmp/ipcr_exc_ab_r.fa"}


def make(gbases):
    import numpy as np
    rng = np.random.default_rng(7)
    n = int(gbases * 1e9)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    for p in rng.integers(0, n - 1000, n // 100_000):  # N runs of 1..1000: ~0.5 % of the bases
        seq[p:p + int(rng.integers(1, 1001))] = ord("N")
    for name, path in FILES.items():
        s = seq.copy()
        if name == "iupac_10kb":
            s[5000::10_000] = ord("R")
        with open(path, "wb") as fh:
            per = n // 8
            for r in range(8):
                part = s[r * per:(r + 1) * per]
                fh.write(b">chr%d synthetic\n" % (r + 1))
                body = np.empty((len(part) // 80, 81), dtype=np.uint8)
                body[:, :80] = part[: (len(part) // 80) * 80].reshape(-1, 80)
                body[:, 80] = 10
                fh.write(body.tobytes())
                rest = part[(len(part) // 80) * 80:]
                if len(rest):
                    fh.write(rest.tobytes() + b"\n")


def child(lib_path, path, gbases, reps):
    lib = C.CDLL(lib_path)
    lib.ipcr_genome_create.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.ipcr_genome_add_fasta.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.c_uint64, C.c_void_p]
    lib.ipcr_genome_destroy.argtypes = [C.c_void_p]
    best = None
    for _ in range(reps):
        h = C.c_void_p()
        assert lib.ipcr_genome_create(int(gbases * 1e9) + (1 << 22), 16, C.byref(h)) == 0
        n = C.c_uint32()
        t0 = time.perf_counter()
        assert lib.ipcr_genome_add_fasta(h, path.encode(), C.byref(n), None, 0, None) == 0
        ms = (time.perf_counter() - t0) * 1e3
        lib.ipcr_genome_destroy(h)
        best = ms if best is None else min(best, ms)
    print(json.dumps({"ms": round(best, 2)}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], float(sys.argv[4]), int(sys.argv[5]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs="+", help="LABEL=path of libipcr_hip.so")
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    builds = [b.split("=", 1) for b in a.builds]
    make(a.gbases)
    res = {}
    for rnd in range(a.rounds):
        for fname, path in FILES.items():
            for loader in ("default", "device"):
                order = builds if rnd % 2 == 0 else builds[::-1]
                for label, lib_path in order:
                    env = dict(os.environ)
                    if loader == "device":
                        env["IPCR_FASTA_HOSTPACK"] = "0"
                    out = subprocess.run([sys.executable, __file__, "--child", os.path.abspath(lib_path), path, str(a.gbases), str(a.reps)],
                                         env=env, capture_output=True, text=True, timeout=300)
                    if out.returncode != 0:
                        sys.stderr.write(out.stderr)
                        sys.exit(out.returncode)
                    ms = json.loads(out.stdout.strip().splitlines()[-1])["ms"]
                    res.setdefault("%s/%s/%s" % (fname, loader, label), []).append(ms)
                    print("round %d  %-10s %-7s %-6s %8.2f ms" % (rnd, fname, loader, label, ms), flush=True)
    summary = {"gbases": a.gbases, "rounds": a.rounds, "reps_per_child": a.reps, "load_ms_min_per_child": res,
               "load_ms_median": {k: sorted(v)[len(v) // 2] for k, v in res.items()}}
    print(json.dumps(summary["load_ms_median"], indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    for p in FILES.values():
        os.unlink(p)


if __name__ == "__main__":
    main()
