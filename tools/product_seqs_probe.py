"""ipcr_genome_read_windows on a large resident genome: wall time and GB/s of one call over N windows of 1-2 kb.

    python tools/product_seqs_probe.py [--gbases 3] [--windows 1000000] [--iupac-every 0] [--out profiles/r06_read_windows.json]

The genome is the benchmark's LCG stream (24 records of 125 Mb for 3 Gb), generated on the device.  With --iupac-every K a
byte 'R' is planted every K bases (exception runs for the read to restore).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/product_seqs_probe.py ...` to see gather_amplicons_kernel against the
device-to-host copies."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=3.0)
    ap.add_argument("--windows", type=int, default=1_000_000)
    ap.add_argument("--iupac-every", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from ipcr_amd import _lib, engine
    rec_len = 125_000_000
    nrec = max(1, int(a.gbases * 1e9) // rec_len)
    g = engine.Genome(nrec * (rec_len + 8192), nrec)
    buf = torch.empty(rec_len, dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    for r in range(nrec):
        _lib.check(_lib.lib().ipcr_lcg_fill_device(buf.data_ptr(), rec_len, 1, r * rec_len))
        if a.iupac_every:
            buf[a.iupac_every // 2::a.iupac_every] = ord("R")
            torch.cuda.synchronize()
        g.add_record_device("r%d" % r, buf.data_ptr(), rec_len)
    load_s = time.perf_counter() - t0
    rng = random.Random(1)
    win = []
    for _ in range(a.windows):
        ln = rng.randrange(1000, 2001)
        s = rng.randrange(rec_len - ln)
        win.append((rng.randrange(nrec), s, s + ln))
    total = sum(e - s for _, s, e in win)
    runs = g.exception_runs
    import ctypes as C
    arr = (_lib.Window * len(win))()
    for i, (r, s, e) in enumerate(win):
        arr[i].record, arr[i].start, arr[i].end = r, s, e
    offs = (C.c_uint64 * (len(win) + 1))()
    need = C.c_uint64()
    out = (C.c_uint8 * total)()
    call = _lib.lib().ipcr_genome_read_windows
    _lib.check(call(g._h, arr, 1000, out, total, offs, C.byref(need)))  # (first use: the context's buffers)
    times = []
    for _ in range(a.reps):  # the C call alone: no Python lists of bytes
        t = time.perf_counter()
        _lib.check(call(g._h, arr, len(win), out, total, offs, C.byref(need)))
        times.append(time.perf_counter() - t)
    assert need.value == total
    assert g.read_windows(win[:3]) == [bytes(out[offs[i]:offs[i + 1]]) for i in range(3)]
    res = {"genome_bases": nrec * rec_len, "records": nrec, "windows": len(win), "bytes": total, "exception_runs": runs,
           "load_s": round(load_s, 3), "read_s": [round(t, 4) for t in times], "read_s_min": round(min(times), 4),
           "gb_per_s": round(total / min(times) / 1e9, 3)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
