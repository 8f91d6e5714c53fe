#!/usr/bin/env python3
"""dev tool (GPU box): the primer-site read on a large resident genome, against the only route the parent build has to the
same bytes -- ipcr_genome_read_windows over the same short windows plus the reverse complement on the host.  A / B / A / B
in fresh child processes, as tools/fasta_load_exc_ab.py does.

    python3 tools/sites_probe.py A=path/to/parent/libipcr_hip.so B=ipcr_amd/libipcr_hip.so [--gbases 3] [--sites 2000000]
                                 [--rounds 3] [--out profiles/r08_sites_probe.json]

Workload: the benchmark's LCG genome (records of 125 Mb, generated on the device); `--sites` sites of 20 nt at positions
from a fixed-seed generator, every second one reverse-complemented; then the same genome with an 'R' every 10 kb, so that
the exception path is in the numbers.  Build A runs `windows` (read_windows + host complement), build B runs `sites`
(ipcr_genome_read_sites) and `windows` too; B's two results are compared byte for byte.  The children call the C ABI through
ctypes directly, so a build without the newer symbols loads.  For the split into kernel and copy time run one child under
`rocprofv3 --kernel-trace --memory-copy-trace --stats -- python3 tools/sites_probe.py --child LIB sites 3 2000000 0 3`."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

REC_LEN = 125_000_000
SITE_LEN = 20


class Window(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("record", C.c_int32), ("reserved", C.c_int32)]


class Site(C.Structure):
    _fields_ = [("pos", C.c_int64), ("record", C.c_int32), ("len", C.c_uint16), ("revcomp", C.c_uint16)]


def child(lib_path, mode, gbases, nsites, iupac_every, reps):
    import numpy as np
    import torch                                         # (first: the library binds to the HIP runtime torch loaded)
    lib = C.CDLL(lib_path)
    lib.ipcr_genome_create.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.ipcr_genome_add_record_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.ipcr_lcg_fill_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64]
    lib.ipcr_genome_read_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.ipcr_last_error.restype = C.c_char_p
    nrec = max(1, int(gbases * 1e9) // REC_LEN)
    g = C.c_void_p()
    assert lib.ipcr_genome_create(nrec * (REC_LEN + 8192), nrec, C.byref(g)) == 0, lib.ipcr_last_error()
    buf = torch.empty(REC_LEN, dtype=torch.uint8, device="cuda")
    for r in range(nrec):
        assert lib.ipcr_lcg_fill_device(buf.data_ptr(), REC_LEN, 1, r * REC_LEN) == 0
        if iupac_every:
            buf[iupac_every // 2::iupac_every] = ord("R")
        torch.cuda.synchronize()
        assert lib.ipcr_genome_add_record_device(g, buf.data_ptr(), REC_LEN) == 0, lib.ipcr_last_error()
    rng = np.random.default_rng(20)
    rec = rng.integers(0, nrec, nsites, dtype=np.int32)
    pos = rng.integers(0, REC_LEN - SITE_LEN, nsites, dtype=np.int64)
    total = nsites * SITE_LEN
    offs = (C.c_uint64 * (nsites + 1))()
    need = C.c_uint64()
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGTRYSWKMBVDHN", b"TGCAYRSWMKVBHDN"):
        comp[a] = b

    def windows_call():
        w = np.zeros(nsites, dtype=np.dtype([("start", "<i8"), ("end", "<i8"), ("record", "<i4"), ("reserved", "<i4")]))
        w["start"], w["end"], w["record"] = pos, pos + SITE_LEN, rec
        out = np.empty(total, dtype=np.uint8)

        def call(n):
            st = lib.ipcr_genome_read_windows(g, w.ctypes.data, n, out.ctypes.data, total, offs, C.byref(need))
            assert st == 0, lib.ipcr_last_error()
            v = out[:n * SITE_LEN].reshape(-1, SITE_LEN)
            v[1::2] = comp[v[1::2, ::-1]]               # the host's part: every second site reverse-complemented
        return call, out

    def sites_call():
        lib.ipcr_genome_read_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        s = np.zeros(nsites, dtype=np.dtype([("pos", "<i8"), ("record", "<i4"), ("len", "<u2"), ("revcomp", "<u2")]))
        s["pos"], s["record"], s["len"] = pos, rec, SITE_LEN
        s["revcomp"][1::2] = 1
        out = np.empty(total, dtype=np.uint8)

        def call(n):
            st = lib.ipcr_genome_read_sites(g, s.ctypes.data, n, out.ctypes.data, total, offs, C.byref(need))
            assert st == 0, lib.ipcr_last_error()
        return call, out

    call, out = (sites_call if mode == "sites" else windows_call)()
    call(1000)                                           # first use: the context's buffers
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call(nsites)
        times.append(time.perf_counter() - t)
    res = {"mode": mode, "s": [round(t, 4) for t in times], "s_min": round(min(times), 4)}
    if mode == "sites":                                  # the same bytes as the parent's route, in this build
        other, want = windows_call()
        other(nsites)
        res["equal_to_windows_route"] = bool((out == want).all())
        res["bytes_outside_acgt"] = int((~np.isin(out, np.frombuffer(b"ACGT", dtype=np.uint8))).sum())
    print(json.dumps(res))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], float(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs=2, help="A=parent libipcr_hip.so B=this build's")
    ap.add_argument("--gbases", type=float, default=3.0)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    builds = dict(b.split("=", 1) for b in a.builds)
    runs = [("A", "windows"), ("B", "sites"), ("B", "windows")]
    res, equal = {}, []
    for rnd in range(a.rounds):
        for variant, every in (("acgt", 0), ("iupac_10kb", 10_000)):
            for label, mode in (runs if rnd % 2 == 0 else runs[::-1]):
                out = subprocess.run([sys.executable, __file__, "--child", os.path.abspath(builds[label]), mode, str(a.gbases),
                                      str(a.sites), str(every), str(a.reps)], capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    sys.stderr.write(out.stderr)
                    sys.exit(out.returncode)
                r = json.loads(out.stdout.strip().splitlines()[-1])
                res.setdefault("%s/%s/%s" % (variant, label, mode), []).append(r["s_min"])
                if "equal_to_windows_route" in r:
                    equal.append(r["equal_to_windows_route"])
                print("round %d  %-10s %s %-7s %8.4f s" % (rnd, variant, label, mode, r["s_min"]), flush=True)
    summary = {"gbases": a.gbases, "sites": a.sites, "site_len": SITE_LEN, "rounds": a.rounds, "reps_per_child": a.reps,
               "call_s_min_per_child": res, "call_s_median": {k: sorted(v)[len(v) // 2] for k, v in res.items()},
               "call_s_range": {k: [min(v), max(v)] for k, v in res.items()}, "sites_equal_windows_route": all(equal) and bool(equal)}
    print(json.dumps(summary["call_s_median"], indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
