"""Chained scans on two lanes (ipcr_scratch_chain_after, IPCR_CHAIN_LANES): consecutive sweeps of a chain run on
alternating streams with no dependency between them, so scratches must share nothing -- hit buffers, counters, tickets,
pinned blocks, timing events.  Every case runs on both forms of the specialised filter: the one small launches take
(several waves share a block) and the whole-block kernel (IPCR_JIT_SEG_BLOCKS=0, read per launch)."""
import ctypes
import random
import time

import pytest

import ipcr_oracle as O

pytestmark = pytest.mark.gpu

REC_LENS = (300_017, 299_983, 301_111)   # a handful of blocks, none a multiple of the block


def _plant(rng, seq, primer_seq, pos, nmut):
    s = list(primer_seq)
    for _ in range(nmut):
        j = rng.randrange(len(s))
        s[j] = O.different_base(s[j])
    seq[pos:pos + len(s)] = s


class World:
    pass


def _inputs():
    """(host only) two small panels, three records with planted amplicons of both, the oracle's products of each panel"""
    from ipcr_amd import primer, workloads
    rng = random.Random(808)
    ocfg = O.Config(max_mm=2, terminal_window=5, max_len=2000, hit_cap=10000, seed_len=12)
    panels = [primer.AddSelfPairs([workloads.bench_pair(0)]),
              primer.AddSelfPairs([workloads.bench_pair(3), workloads.bench_pair(4)])]
    stream = O.bench_dna(sum(REC_LENS), 0x5eed0808)
    seqs, off = [], 0
    for r, n in enumerate(REC_LENS):
        s = list(stream[off:off + n].decode())
        off += n
        for t in range(8):                       # panel 0: 8 sites per record, panel 1: 4 + 3
            a = 1500 + t * 35_000 + rng.randrange(700)
            pr = panels[0][0]
            _plant(rng, s, pr.Forward, a, rng.choice([0, 1, 2]))
            _plant(rng, s, O.revcomp(pr.Reverse).decode(), a + 170, rng.choice([0, 1]))
            if t < 7:
                pr = panels[1][0] if t < 4 else panels[1][1]
                _plant(rng, s, pr.Forward, a + 9000, rng.choice([0, 1]))
                _plant(rng, s, O.revcomp(pr.Reverse).decode(), a + 9000 + 150, 0)
        seqs.append("".join(s).encode())
    wants = []
    for p in panels:
        op = O.Panel(ocfg, [O.Pair(q.ID, q.Forward, q.Reverse, q.MinProduct, q.MaxProduct) for q in p])
        wants.append([("chr%d" % r,) + x.sig() for r, s in enumerate(seqs) for x in op.scan(s)])
    # (a mismatch planted inside the 3' window costs a site its product: the counts are what the oracle says)
    assert min(map(len, wants)) >= 10 and len(wants[0]) != len(wants[1])
    return panels, seqs, wants


@pytest.fixture(scope="module")
def world():
    """the genome on the device, the compiled panels and the oracle's products of each -- made once"""
    from ipcr_amd import _lib, engine
    assert _lib.lib().ipcr_device_count() > 0, "needs a HIP device"
    w = World()
    w.lib, w.engine = _lib, engine
    panels, seqs, w.want = _inputs()
    w.cfg = engine.Config(MaxMM=2, TerminalWindow=5, MaxLen=2000, HitCap=10000, SeedLen=12)
    w.g = engine.Genome(sum(REC_LENS) + 65536, max_records=4)
    for r, s in enumerate(seqs):
        w.g.add_record("chr%d" % r, s)
    w.eng = engine.New(w.cfg)
    w.cps = [w.eng.CompilePanel(p) for p in panels]
    w.lane = _lib.lib().ipcr_internal_scratch_lane
    w.lane.restype = ctypes.c_void_p
    w.lane.argtypes = [ctypes.c_void_p]
    for cp in w.cps:                              # (a small panel's kernels are built in the background: wait for both forms' source)
        sc = w.eng.NewSimulationScratch(cp)
        w.eng.ScanGenomeCount(w.g, cp, sc)
        cp.wait_ready()
        sc.close()
    yield w
    w.g.close()


@pytest.fixture(params=("small-launch form", "whole-block kernel"))
def form(request, monkeypatch):
    if request.param == "whole-block kernel":
        monkeypatch.setenv("IPCR_JIT_SEG_BLOCKS", "0")
    return request.param


def _sigs(sc, g):
    return [(p.SequenceID,) + p.sig() for p in sc.products(g.ids)]


def _chained_passes(w, scs, cps, k, each=None):
    """k pipelined passes over the scratches in rotation, as bench.py runs them: pass i+1 is chained after pass i and
    begun before pass i is ended.  each(i, scratch) after every end.  -> the lanes the passes ran on"""
    ns, lanes = len(scs), []
    w.eng.ScanGenomeBegin(w.g, cps[0], scs[0])
    lanes.append(w.lane(scs[0]._h))
    for i in range(k):
        if i + 1 < k:
            j = (i + 1) % ns
            scs[j].chain_after(scs[i % ns])
            w.eng.ScanGenomeBegin(w.g, cps[j], scs[j])
            lanes.append(w.lane(scs[j]._h))
        n = w.eng.ScanGenomeEndCount(w.g, cps[i % ns], scs[i % ns])
        if each is not None:
            each(i, scs[i % ns], n)
    return lanes


@pytest.mark.parametrize("nscratch", (3, 2))
def test_chained_passes_equal_the_oracle(world, form, nscratch):
    """(a) 24 chained passes, the two panels alternating per scratch: every pass gives its own panel's products -- the
    oracle's, and those of an unchained scan.  A hit buffer, a counter set or a pinned block mixed up between the lanes
    shows as the other panel's products (their counts differ)."""
    w = world
    cps = [w.cps[j % 2] for j in range(nscratch)]
    scs = [w.eng.NewSimulationScratch(cp) for cp in cps]
    for j, sc in enumerate(scs):                  # unchained single scans
        got = [(p.SequenceID,) + p.sig() for p in w.eng.ScanGenome(w.g, cps[j], sc)]
        assert got == w.want[j % 2], (form, j)
        assert sc.stats().kernel_kind == 1

    def each(i, sc, n):
        want = w.want[(i % nscratch) % 2]
        assert n == len(want) and _sigs(sc, w.g) == want, (form, nscratch, i)

    lanes = _chained_passes(w, scs, cps, 24, each)
    assert len(set(lanes)) == 2
    for sc in scs:
        sc.close()


def test_lanes_alternate(world, form, monkeypatch):
    """(b) consecutive chained scans run on different lanes -- two in all, the streams of the chain's first two
    scratches; IPCR_CHAIN_LANES=1 keeps the whole chain on one; an unchained scan is back on the scratch's own."""
    w = world
    for nscratch in (3, 2):
        scs = [w.eng.NewSimulationScratch(w.cps[0]) for _ in range(nscratch)]
        cps = [w.cps[0]] * nscratch
        own = []
        for sc in scs:
            w.eng.ScanGenomeCount(w.g, w.cps[0], sc)
            own.append(w.lane(sc._h))
        assert len(set(own)) == nscratch and None not in own
        lanes = _chained_passes(w, scs, cps, 9)
        assert all(a != b for a, b in zip(lanes, lanes[1:])), lanes
        assert lanes[0] == own[0] and lanes[1] == own[1] and set(lanes) == {own[0], own[1]}, (lanes, own)
        monkeypatch.setenv("IPCR_CHAIN_LANES", "1")
        lanes = _chained_passes(w, scs, cps, 9)
        assert set(lanes) == {own[0]}, (lanes, own)
        monkeypatch.delenv("IPCR_CHAIN_LANES")
        lanes = _chained_passes(w, scs, cps, 4)      # and back, from whatever the one-lane chain left behind
        assert all(a != b for a, b in zip(lanes, lanes[1:])), lanes
        for j, sc in enumerate(scs):
            w.eng.ScanGenomeCount(w.g, w.cps[0], sc)
            assert w.lane(sc._h) == own[j]
        for sc in scs:
            sc.close()


@pytest.fixture(scope="module")
def dense():
    """a genome whose poly-A record gives a k = 1 poly-A panel more raw hits than a fresh hit buffer holds (1 Mi records:
    three patterns match at every one of its 600 k positions),
    next to two ordinary records; the oracle's products of that panel"""
    from ipcr_amd import engine, primer, workloads
    P = primer.Pair
    rng = random.Random(4242)
    recs = []
    for r in range(3):
        if r == 1:
            s = bytearray(b"A" * 600_011)
            for _ in range(30):
                s[rng.randrange(len(s))] = rng.choice(b"CGTN")
            s[1000:1012] = b"TTTTTTTTTTTT"
        else:
            s = bytearray(O.bench_dna(120_003, 0x5eed0d00 + r))
            s[5000:5040] = b"A" * 40
            for t, i in enumerate((0, 3, 4, 0, 3)):   # sites of the two sparse panels of `world`
                pr = workloads.bench_pair(i)
                s[20_000 * (t + 1):20_000 * (t + 1) + 20] = pr.Forward.encode()
                s[20_000 * (t + 1) + 140:20_000 * (t + 1) + 160] = O.revcomp(pr.Reverse)
        recs.append(bytes(s))
    pairs = [P("polyA", "AAAAAAAAAAAA", "TTTTTTTTTTTT"), P("mixed", "AAAAAACAAAAA", "TTTTTTTTTTGT")]
    cfg = engine.Config(MaxMM=1, TerminalWindow=3, MaxLen=60, HitCap=50, SeedLen=12)
    ocfg = O.Config(max_mm=1, terminal_window=3, max_len=60, hit_cap=50, seed_len=12)
    opairs = [O.Pair(p.ID, p.Forward, p.Reverse, p.MinProduct, p.MaxProduct) for p in pairs]
    want = []
    for r, s in enumerate(recs):
        want += [("r%d" % r,) + x.sig() for x in O.simulate_batch(ocfg, s, opairs)]
    assert len(want) >= 10
    return recs, pairs, cfg, want


def test_overflow_redo_while_chained(world, form, dense):
    """(c) the middle scratch of a chain scans with a panel whose raw hits overflow its fresh hit buffer: its first chained
    pass regrows the buffer and repeats the sweep (on the scratch's own stream, after the first attempt has retired) while
    its successor's sweep is already queued on the other lane.  It still equals the oracle, and so do the passes of the
    other scratches before and after it."""
    w = world
    recs, pairs, cfg, want_dense = dense
    g = w.engine.Genome(sum(map(len, recs)) + 65536, max_records=4)
    for r, s in enumerate(recs):
        g.add_record("r%d" % r, s)
    eng_d = w.engine.New(cfg)
    cp_d = eng_d.CompilePanel(pairs)
    warm = eng_d.NewSimulationScratch(cp_d)       # builds the panel's kernels; this scratch's buffer regrows, the chain's is fresh
    assert [(p.SequenceID,) + p.sig() for p in eng_d.ScanGenome(g, cp_d, warm)] == want_dense
    cp_d.wait_ready()
    assert warm.stats().hits > (1 << 20) and warm.stats().segmented == 0
    warm.close()
    # the chain: sparse panel, dense panel, sparse panel -- all over the dense genome
    eng = w.eng
    cps = [w.cps[0], cp_d, w.cps[1]]
    ocfg = O.Config(max_mm=2, terminal_window=5, max_len=2000, hit_cap=10000, seed_len=12)
    wants = []
    for cp in cps:
        if cp is cp_d:
            wants.append(want_dense)
            continue
        opairs = [O.Pair(q.ID, q.Forward, q.Reverse, q.MinProduct, q.MaxProduct) for q in cp.Pairs]
        wants.append([("r%d" % r,) + x.sig() for r, s in enumerate(recs) for x in O.simulate_batch(ocfg, s, opairs)])
        assert len(wants[-1]) >= 4
    scs = [eng.NewSimulationScratch(cp) for cp in cps]
    caps = []

    def begin(j):
        eng.ScanGenomeBegin(g, cps[j], scs[j])

    def end(j):
        return eng.ScanGenomeEndCount(g, cps[j], scs[j])

    assert scs[1].device_hits()[2] == 1 << 20
    begin(0)
    for i in range(9):
        if i + 1 < 9:
            j = (i + 1) % 3
            scs[j].chain_after(scs[i % 3])
            begin(j)
        n = end(i % 3)
        assert n == len(wants[i % 3]) and _sigs(scs[i % 3], g) == wants[i % 3], (form, i)
        if i % 3 == 1:
            caps.append(scs[1].device_hits()[2])
            assert scs[1].stats().hits > (1 << 20)
    assert caps[0] > (1 << 20) and caps == [caps[0]] * 3   # pass 1 regrew it; passes 4 and 7 found it large enough
    for sc in scs:
        sc.close()
    cp_d.close()
    g.close()


def test_exclusive_time_accounting(world, form, monkeypatch):
    """(d) filter_ms of a scan chained on the other lane is the time by which its sweep extended the device's busy
    period: over a window of chained passes the values sum to no more than the window's wall time, and every one is
    positive (equal sweeps: the one enqueued later ends later).  On one lane they are the launches' own times, as those
    of unchained scans are."""
    w = world
    scs = [w.eng.NewSimulationScratch(w.cps[0]) for _ in range(3)]
    cps = [w.cps[0]] * 3
    solo = []
    for sc in scs:
        for _ in range(3):
            w.eng.ScanGenomeCount(w.g, w.cps[0], sc)
            solo.append(sc.stats().filter_ms)
    assert min(solo) > 0
    for lanes in ("2", "1"):
        monkeypatch.setenv("IPCR_CHAIN_LANES", lanes)
        _chained_passes(w, scs, cps, 6)               # warm
        fms = []
        t0 = time.perf_counter()
        _chained_passes(w, scs, cps, 24, lambda i, sc, n: fms.append(sc.stats().filter_ms))
        wall_ms = (time.perf_counter() - t0) * 1e3
        print("lanes=%s form=%s: sum filter_ms %.4f, wall %.4f ms, min %.5f max %.5f, solo %.5f..%.5f"
              % (lanes, form, sum(fms), wall_ms, min(fms), max(fms), min(solo), max(solo)))
        assert len(fms) == 24 and min(fms) > 0, fms
        assert sum(fms) <= wall_ms, (sum(fms), wall_ms)
        # the same kernel over the same tiles: clocks and a co-running sweep move a launch of some 10 us by tens of per
        # cent, not by 3x.  One lane: the launches' own times, i.e. what the sweep takes alone; two: never more than that
        med, med_solo = sorted(fms)[12], sorted(solo)[len(solo) // 2]
        assert med <= 3.0 * med_solo, (fms, solo)
        if lanes == "1":
            assert med >= med_solo / 3.0, (fms, solo)
    for sc in scs:
        sc.close()


def test_handover_check_over_two_lanes(world, form, monkeypatch):
    """(e) IPCR_DEBUG_PUBLISH_CHECK=1 over chained two-lane passes: what the host took from each scratch's pinned block is
    what that scratch's sweep left in device memory -- 0 differences, nothing refetched."""
    w = world
    monkeypatch.setenv("IPCR_DEBUG_PUBLISH_CHECK", "1")
    cps = [w.cps[0], w.cps[1], w.cps[0]]
    scs = [w.eng.NewSimulationScratch(cp) for cp in cps]
    tot = {"checked": 0, "diffs": 0, "refetched": 0}

    def each(i, sc, n):
        st = sc.stats()
        assert n == len(w.want[(i % 3) % 2])
        tot["checked"] += st.handover_checked
        tot["diffs"] += st.handover_check_diffs
        tot["refetched"] += st.handover_refetched

    lanes = _chained_passes(w, scs, cps, 12, each)
    assert len(set(lanes)) == 2
    assert tot == {"checked": 12, "diffs": 0, "refetched": 0}, tot
    for sc in scs:
        sc.close()
