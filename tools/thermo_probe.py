#!/usr/bin/env python3
"""dev tool (GPU box): the thermo score of many products, on the device against the host route.

    python3 tools/thermo_probe.py [--model legacy-heuristic|nn-duplex-v1] [--products 100000] [--reps 5] [--out profiles/r09_thermo_probe.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/thermo_probe.py --child device 100000 5 [nn-duplex-v1]    (kernel time, own run)

Workload: one resident record of `--products` planted amplicons (a 20-nt and a 22-nt primer, 0-2 mismatches per site, 60
bases between them, 40 bases of spacer), scanned once; the products stay in the scratch.  Timed per repetition, after one
warm-up call of each route:
  device   ipcr_thermo_legacy_products: one call, one double per product comes back
  host     the route a build without that call has to the same scores: ipcr_product_sites (the 2 x 20-odd window bytes of
           every product over the link), then the complement and ipcr_thermo_legacy_penalty per end on the host
With --model nn-duplex-v1 the device route is ipcr_thermo_nn_duplex_products (scores only) and the host route
ipcr_thermo_nn_duplex_end per end, the base next to each window taken from the record this tool built.
The two results are compared bit for bit.  Each route runs in a child process of its own (fresh runtime, as
tools/sites_probe.py does); the parent alternates them."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def build_record(n, seed=31):
    import numpy as np
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    F, Rv = acgt[rng.integers(0, 4, 20)], acgt[rng.integers(0, 4, 22)]
    rc_rv = np.frombuffer(bytes(Rv)[::-1].translate(COMP), dtype=np.uint8)
    unit = 20 + 60 + 22 + 40
    rec = acgt[rng.integers(0, 4, n * unit)].reshape(n, unit).copy()
    rec[:, :20] = F
    rec[:, 80:102] = rc_rv
    for col0, width in ((0, 20), (80, 22)):                 # 0-2 mismatches per site (a changed base may equal the old one)
        for _ in range(2):
            rows = np.nonzero(rng.random(n) < 0.5)[0]
            rec[rows, col0 + rng.integers(0, width, rows.size)] = acgt[rng.integers(0, 4, rows.size)]
    return bytes(F).decode(), bytes(Rv).decode(), rec.tobytes()


def child(mode, n, reps, model="legacy-heuristic"):
    sys.path.insert(0, ROOT)
    from ipcr_amd import _lib, engine, primer, thermo
    F, Rv, rec = build_record(n)
    eng = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=0, MaxLen=150, SeedLen=12))
    cp = eng.CompilePanel([primer.Pair("p", F, Rv)])
    sc = eng.NewSimulationScratch(cp)
    g = engine.Genome(len(rec) + (1 << 20), 2)
    g.add_record("r", rec)
    nprod = eng.ScanGenomeCount(g, cp, sc)
    L = _lib.lib()
    out = (C.c_double * nprod)()

    def device():
        _lib.check(L.ipcr_thermo_legacy_products(sc._h, g._h, None, 0, out, nprod))
        return list(out)

    def host():
        sites = sc.product_sites(g)                         # (FwdSite, RevSite = reverse complement of the right window)
        pen, res, o = L.ipcr_thermo_legacy_penalty, [], C.c_double()
        f, r = F.encode(), Rv.encode()
        for fs, rs in sites:                                # complement, not reversed, at both ends
            pen(f, fs.encode().translate(COMP), 200.0, C.byref(o))
            a = o.value
            pen(r, rs.encode()[::-1], 200.0, C.byref(o))    # comp(window) = reverse(revcomp(window))
            res.append(-(a + o.value))
        return res

    nn = model == "nn-duplex-v1"
    if nn:
        pairs = [primer.Pair("p", F, Rv)]
        base = thermo.panel_nn_base(pairs, thermo.DefaultConditions())
        tab = (_lib.ThermoNNPrimer * 2)(*(_lib.ThermoNNPrimer(t, d) for t, d in base))
        prods = sc.products(["r"])

    def device_nn():
        _lib.check(L.ipcr_thermo_nn_duplex_products(sc._h, g._h, tab, 2, 60.0, out, None, nprod))
        return list(out)

    def host_nn():
        sites = sc.product_sites(g)                         # (FwdSite, RevSite = reverse complement of the right window)
        end, res, o = L.ipcr_thermo_nn_duplex_end, [], _lib.ThermoNNEnd()
        for p, (fs, rs) in zip(prods, sites):               # (forward products only: the panel has one pair, planted one way)
            lp, rp, bl, br = (F, Rv, base[0], base[1]) if p.Type == "forward" else (Rv, F, base[1], base[0])
            a, b = p.Start + len(lp), p.End - len(rp) - 1   # the amplicon's base behind the left / before the right window
            dl = rec[a:a + 1].translate(COMP) if a < p.End else b"\0"
            dr = rec[b:b + 1] if b >= p.Start else b"\0"
            end(lp.encode(), fs.encode().translate(COMP), dl, bl[0], bl[1], C.byref(o))
            left = o.tm_c - 60.0
            end(rp.encode(), rs.encode().translate(COMP), dr, br[0], br[1], C.byref(o))   # reverse(window) = comp(revcomp(window))
            right = o.tm_c - 60.0
            res.append(right if right < left else left)
        return res

    if nn:
        device, host = device_nn, host_nn
    fn = device if mode == "device" else host
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        got = fn()
        times.append(time.perf_counter() - t)
    import struct
    other = host() if mode == "device" else device()
    same = struct.pack("<%dd" % nprod, *got) == struct.pack("<%dd" % nprod, *other)
    print(json.dumps({"mode": mode, "products": nprod, "s": [round(t, 5) for t in times], "s_min": round(min(times), 5),
                      "equal_to_other_route_bitwise": same, "distinct_scores": len(set(got))}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), *sys.argv[5:6])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--products", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--model", default="legacy-heuristic", choices=("legacy-heuristic", "nn-duplex-v1"))
    a = ap.parse_args()
    res, info = {"device": [], "host": []}, {}
    for rnd in range(a.rounds):
        for mode in (("device", "host") if rnd % 2 == 0 else ("host", "device")):
            out = subprocess.run([sys.executable, __file__, "--child", mode, str(a.products), str(a.reps), a.model], capture_output=True,
                                 text=True, timeout=900)
            if out.returncode != 0:
                sys.stderr.write(out.stderr)
                sys.exit(out.returncode)
            r = json.loads(out.stdout.strip().splitlines()[-1])
            res[mode].append(r["s_min"])
            info[mode] = r
            print("round %d  %-6s %9.5f s  (%d products, bitwise equal to the other route: %s)" %
                  (rnd, mode, r["s_min"], r["products"], r["equal_to_other_route_bitwise"]), flush=True)
    summary = {"model": a.model, "products": info["device"]["products"], "rounds": a.rounds, "reps_per_child": a.reps,
               "call_s_min_per_child": res, "call_s_median": {k: sorted(v)[len(v) // 2] for k, v in res.items()},
               "call_s_range": {k: [min(v), max(v)] for k, v in res.items()},
               "bitwise_equal": all(info[m]["equal_to_other_route_bitwise"] for m in info),
               "distinct_scores": info["device"]["distinct_scores"]}
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
