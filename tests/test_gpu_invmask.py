"""The genome's column mask (which columns hold an invalid base) and the specialised filter that skips the inv plane of
the other columns (IPCR_JIT_INVMASK, jit.cpp).  The mask is checked bit for bit against a recompute from the records'
bases for every tile writer; scans with the knob on are compared with the oracle and with the knob off."""
import ctypes
import random

import pytest

import ipcr_oracle as O

pytestmark = pytest.mark.gpu

COL = 4096  # bases per column (tile_layout.h)


def record_cols(n):
    return (n + 128 + 8191) // 8192 * 2


def read_mask(g):
    from ipcr_amd import _lib
    f = _lib.lib().ipcr_internal_genome_column_mask
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    n = f(g._h, None, 0)
    assert n > 0
    buf = (ctypes.c_uint64 * n)()
    assert f(g._h, buf, n) == n
    return list(buf)


def expected_mask(g, nwords):
    """bit set = the column holds a base that is not an upper-case ACGT (what the inv plane holds); columns behind the
    records are padding or never written: dirty"""
    want = [(1 << 64) - 1] * nwords
    col = 0
    for r in range(g.num_records):
        n = g.record_len(r)
        seq = g.read(r, 0, n)
        for c in range(record_cols(n)):
            piece = seq[c * COL:(c + 1) * COL]
            dirty = len(piece) < COL or piece.translate(None, b"ACGT") != b""
            if not dirty:
                want[(col + c) // 64] &= ~(1 << ((col + c) % 64))
        col += record_cols(n)
    return want


def check_mask(g, what):
    got = read_mask(g)
    want = expected_mask(g, len(got))
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, (what, [(i, hex(got[i]), hex(want[i])) for i in bad[:4]])


def acgt(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def plant(seq, pos, ch):
    b = bytearray(seq)
    b[pos] = ch
    return bytes(b)


def records(rng):
    """clean and dirty records: single invalid bases at lane 0 / lane 63 / row 0 / row 127 of a strand, a run of N, lower case"""
    out = [acgt(rng, 300_000)]                                  # clean but for its last column (record padding)
    s = acgt(rng, 600_000)
    for pos in (0, 63 * COL + 127, 64 * COL, 5 * COL + 31 * 128 + 127, 262_144 * 2 - 1 if len(s) > 524_288 else 1):
        s = plant(s, pos, ord("N"))
    out.append(s)
    s = acgt(rng, 270_000)
    s = s[:100_000] + b"N" * 1000 + s[101_000:]
    out.append(s)
    s = acgt(rng, 20_000)
    out.append(plant(s, 12_345, ord("a")))
    out.append(acgt(rng, 8192 - 128))                          # exactly one column pair, padding included
    return out


def test_mask_add_record():
    from ipcr_amd import engine
    recs = records(random.Random(1))
    g = engine.Genome(sum(record_cols(len(s)) for s in recs) * COL, len(recs))
    for i, s in enumerate(recs):
        g.add_record("r%d" % i, s)
        check_mask(g, "add_record %d" % i)
    g.close()


def test_mask_add_record_device():
    import torch
    from ipcr_amd import engine
    recs = records(random.Random(2))
    g = engine.Genome(sum(record_cols(len(s)) for s in recs) * COL, len(recs))
    for i, s in enumerate(recs):
        buf = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        g.add_record_device("r%d" % i, buf.data_ptr(), len(s))
        del buf
    check_mask(g, "add_record_device")
    g.close()


@pytest.mark.parametrize("nrec", [5, 300])
def test_mask_fasta(tmp_path, nrec):
    """a FASTA load: records of ACGT only, with an N, with lower case; many short records take one batched launch"""
    from ipcr_amd import engine
    rng = random.Random(3 + nrec)
    recs = []
    for i in range(nrec):
        s = acgt(rng, rng.choice((50, 4000, 9000, 70_000)) if nrec > 5 else 300_000)
        if i % 3 == 1:
            s = plant(s, rng.randrange(len(s)), ord("N"))
        if i % 5 == 2:
            s = plant(s, rng.randrange(len(s)), ord("c"))
        recs.append(s)
    path = tmp_path / "g.fa"
    with open(path, "w") as fh:
        for i, s in enumerate(recs):
            fh.write(">r%d\n" % i)
            fh.write("\n".join(s[j:j + 80].decode() for j in range(0, len(s), 80)) + "\n")
    g = engine.Genome(sum(record_cols(len(s)) for s in recs) * COL + 2 * 8192, nrec + 2)
    assert g.add_fasta(str(path)) == nrec
    check_mask(g, "fasta %d" % nrec)
    g.close()


# ---- scans with the knob on and off ------------------------------------------------------------------------------------

def cfg_pairs():
    from ipcr_amd import engine, primer
    rng = random.Random(7)
    fw, rv = acgt(rng, 20).decode(), acgt(rng, 21).decode()
    cfg = engine.Config(MaxMM=2, TerminalWindow=3, MinLen=60, MaxLen=2000, HitCap=0, SeedLen=12)
    return cfg, [primer.Pair("p", fw, rv, 60, 2000)], fw, rv


def ocfg(c):
    return O.Config(max_mm=c.MaxMM, terminal_window=c.TerminalWindow, min_len=c.MinLen, max_len=c.MaxLen,
                    hit_cap=c.HitCap, seed_len=c.SeedLen, circular=c.Circular)


def site_seq(fw, rv, n, starts, subs, rng):
    """n bases with an amplicon at each start; subs: (offset from the amplicon start, byte) written after the sites"""
    from ipcr_amd import primer
    b = bytearray(acgt(rng, n))
    rc = bytes(primer.RevComp(rv))
    for st in starts:
        b[st:st + len(fw)] = fw.encode()
        b[st + 300 - len(rc):st + 300] = rc
        for off, ch in subs:
            b[st + off] = ch
    return bytes(b)


def products(cfg, pairs, seq, scratch_seqs=None):
    from ipcr_amd import engine
    eng = engine.New(cfg)
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    out = []
    for s in (scratch_seqs or [seq]):  # one scratch: its chunk genome is reused
        got = eng.SimulateCompiledWithScratch("s", s, cp, sc)
        assert sc.stats().kernel_kind == 1  # the specialised filter
        out.append([p.sig() for p in got])
    g = engine.Genome(record_cols(len(seq)) * COL, 1)
    g.add_record("s", seq)
    out.append([p.sig() for p in eng.ScanGenome(g, cp, sc)])
    g.close()
    sc.close()
    cp.close()
    return out


def test_scan_knob_parity(monkeypatch):
    """invalid and lower-case bases inside primer sites at lane 0, lane 63, rows 0 and 127 of a strand, column 0 of the
    next block (the wrap neighbour of lane 63) and the record's last column: knob on = knob off = oracle"""
    cfg, pairs, fw, rv = cfg_pairs()
    rng = random.Random(11)
    n = 3 * 262_144 + 5000
    starts = [0, 128 - 5, 63 * COL, 63 * COL + 31 * 128 + 120, 64 * COL - 10, 64 * COL + 3000, 2 * 262_144 - 7, n - 400,
              100_000, 200_000, 300_000]
    seqs = [site_seq(fw, rv, n, starts, [], rng),
            site_seq(fw, rv, n, starts, [(3, ord("N"))], rng),
            site_seq(fw, rv, n, starts, [(0, ord("N")), (19, ord("a")), (150, ord("N"))], rng),
            site_seq(fw, rv, n, starts, [(5, ord("t")), (299, ord("R"))], rng)]
    want = [[w.sig() for w in O.simulate_batch(ocfg(cfg), s, [O.Pair(p.ID, p.Forward, p.Reverse, p.MinProduct, p.MaxProduct)
                                                                for p in pairs])] for s in seqs]
    assert len(want[0]) >= len(starts) - 1
    for knob in ("1", "0"):
        monkeypatch.setenv("IPCR_JIT_INVMASK", knob)
        for s, w in zip(seqs, want):
            for got in products(cfg, pairs, s):
                assert got == w, knob


def test_stale_clean_trap(monkeypatch):
    """a chunk scratch scans a chunk of ACGT only, then one whose exact primer site has N where the primer has A: the
    columns that turned dirty must be read as dirty (an N read as A would be a zero-mismatch hit)"""
    monkeypatch.setenv("IPCR_JIT_INVMASK", "1")
    from ipcr_amd import engine, primer
    rng = random.Random(13)
    fw = "A" + acgt(rng, 19).decode()
    rv = acgt(rng, 20).decode()
    cfg = engine.Config(MaxMM=0, TerminalWindow=0, MinLen=60, MaxLen=2000, HitCap=0, SeedLen=0)
    pairs = [primer.Pair("p", fw, rv, 60, 2000)]
    n = 262_144 + 100_000
    starts = [50_000, 64 * COL + 10, 300_000]
    clean = site_seq(fw, rv, n, starts, [], rng)
    dirty = site_seq(fw, rv, n, starts, [(0, ord("N"))], rng)
    op = [O.Pair(p.ID, p.Forward, p.Reverse, p.MinProduct, p.MaxProduct) for p in pairs]
    want_clean = [w.sig() for w in O.simulate_batch(ocfg(cfg), clean, op)]
    want_dirty = [w.sig() for w in O.simulate_batch(ocfg(cfg), dirty, op)]
    assert len(want_clean) > len(want_dirty)
    got = products(cfg, pairs, dirty, scratch_seqs=[clean, dirty, clean])
    assert got[0] == want_clean and got[1] == want_dirty and got[2] == want_clean
    assert got[3] == want_dirty
