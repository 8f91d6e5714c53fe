"""Hit-level parity: the hit list a scan leaves in its scratch (ipcr_scratch_hits: what dist.py and exchange.cpp gather
between GPUs and join elsewhere) against the exact list of every scanned pattern's matches (test_host_logic.synth_hits),
field for field -- position, record, pattern id with the seed-span reset flag in bit 31, both mismatch-mask words.

Products show a hit only when it pairs with a partner inside MaxLen; the three filter kernels sit in front of an exact
verifier, so a filter that counts too FEW mismatches is invisible and one that counts too MANY loses hits for good.  The
sites here are planted per scanned pattern where the filters' structure changes: every set of k mismatch positions on
short patterns, and for larger k / long patterns all k at the far end, all k next to the enforced window, every other
position, across positions 31/32, 63/64 and 127, all beyond the 20 positions next to the protected end; the same shapes
with k + 1 mismatches, a mismatch inside the window and junk bytes must be absent.  Every table-driven instantiation
(k = 0..16), the specialised filter (in-kernel verifier <= 32 nt, stand-alone verifier beyond, small-launch form), the
seed index and its variants, the cold-cache path, and every way bases reach the device."""
import ctypes
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ipcr_oracle as O
from ipcr_amd import _lib, dist, engine, primer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_logic import synth_hits  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALISED, TABLE, INDEX = 1, 2, 3
P = primer.Pair

# base_match for every genome byte against every primer code (core/primer/iupac.go:62-67 through the oracle)
CODES = "ACGTRYSWKMBDHVN"
MATCH = {p: bytes(1 if O.base_match(chr(g), p) else 0 for g in range(256)) for p in CODES}
JUNK = b"NnRacgt-"   # bytes that match no primer code; N and R are reset bytes, lower case is not


# ---- the match rule, stated once more (tests/test_host_logic.py pins it against the oracle on the CPU) -------------

def window(L, left, tw_dev):
    return set(range(tw_dev)) if left else set(range(L - tw_dev, L))


def site_idx(seq, pos, pat, left, tw_dev, k):
    """the mismatch positions of `pat` at `pos` if it is a hit, else None"""
    L = len(pat)
    if pos < 0 or pos + L > len(seq):
        return None
    idx = tuple(j for j in range(L) if not MATCH[pat[j]][seq[pos + j]])
    if len(idx) > k or window(L, left, tw_dev).intersection(idx):
        return None
    return idx


# ---- sites ---------------------------------------------------------------------------------------------------------

class Site:
    __slots__ = ("rec", "gid", "pos", "subs", "present", "flag", "what")

    def __init__(self, gid, subs, present, what, flag=None):
        self.gid, self.subs, self.present, self.what, self.flag = gid, subs, present, what, flag
        self.rec, self.pos = None, None


def pattern_sites(rng, gid, info, k, dirty, exhaustive):
    """the sites of one scanned pattern: (substitutions {j: byte}, present?, label)"""
    pat, left, tw_dev, soff, slen = info
    L = len(pat)
    win = window(L, left, tw_dev)
    alts = {j: [ord(b) for b in "ACGT" if not MATCH[pat[j]][ord(b)]] for j in range(L)}
    free = [j for j in range(L) if j not in win and alts[j]]
    # distance from the protected end (the end the window sits on, also with tw_dev = 0)
    near = sorted(free, key=lambda j: j if left else L - 1 - j)
    out = []
    cyc = itertools.count()

    def subst(js):
        return {j: alts[j][next(cyc) % len(alts[j])] for j in js}

    def shape(js, what):
        js = list(js)
        if len(js) == k:
            out.append(Site(gid, subst(js), True, what))
        if len(js) == k + 1:
            out.append(Site(gid, subst(js), False, what + " +1"))

    out += [Site(gid, {}, True, "exact") for _ in range(3)]
    if exhaustive:
        for m in range(1, k + 1):
            for js in itertools.combinations(free, m):
                out.append(Site(gid, subst(js), True, "all sets of %d" % m))
    for n in (k, k + 1):
        if n == 0 or n > len(free):
            continue
        shape(near[-n:], "far end")
        shape(near[:n], "next to the window")
        shape(near[::2][:n] if len(near[::2]) >= n else near[-n:], "every other")
        for b in (32, 64, 128):
            if L > b - 1:
                shape(sorted(free, key=lambda j: (abs(j - (b - 0.5)), j))[:n], "around %d" % b)
        beyond = near[20:]
        if len(beyond) >= n:
            shape(beyond[:n], "beyond the 20 filtered")
    if k + 1 <= len(free) and k + 1 > 0:
        shape(rng.sample(free, k + 1), "random +1")
    for w in sorted(win):           # one mismatch inside the enforced window, the rest (total <= k) outside
        if alts[w]:
            rest = near[-(k - 1):] if k > 1 else []
            s = subst(rest)
            s[w] = alts[w][0]
            out.append(Site(gid, s, False, "window base %d" % w))
    if dirty and free:
        j = near[len(near) // 2]
        for b in JUNK[:4]:
            extra = near[-(k - 1):] if k > 1 else []
            s = subst([x for x in extra if x != j])
            s[j] = b
            out.append(Site(gid, s, k >= 1, "junk %r" % chr(b)))
        if slen and k >= 1:          # the reset flag (bit 31): a reset byte inside the seed span against one just outside it
            inside = [j for j in range(soff, soff + slen) if j in free]
            outside = [j for j in (soff - 1, soff + slen) if 0 <= j < L and j in free]
            if inside:
                out.append(Site(gid, {inside[len(inside) // 2]: ord("N")}, True, "N inside the seed span", flag=1))
            for j in outside:
                out.append(Site(gid, {j: ord("N")}, True, "N beside the seed span", flag=0))
    return out


def concrete(rng, pat):
    return bytearray(ord(rng.choice([b for b in "ACGT" if MATCH[c][ord(b)]])) for c in pat)


def put(rng, seq, site, pat, pos):
    b = concrete(rng, pat)
    for j, v in site.subs.items():
        b[j] = v
    seq[pos:pos + len(b)] = b
    site.pos = pos


def background(rng, n):
    return bytearray(rng.choice(b"ACGT") for _ in range(n))


def records_with_sites(rng, cp, mode, k, dirty, exhaustive_max_len=0, nrec=2, gap=7):
    """records of random sequence, every site of every scanned pattern in a slot of its own (spread over `nrec` records);
    dirty: a few junk runs in the gaps as well, so that every record holds a reset byte"""
    sites = []
    for gid in cp.scanned_patterns(mode):
        info = cp.pattern_info(gid)
        ex = len(info[0]) <= exhaustive_max_len
        sites += pattern_sites(rng, gid, info, k, dirty, ex)
    rng.shuffle(sites)
    infos = {g: cp.pattern_info(g) for g in cp.scanned_patterns(mode)}
    per = [sites[r::nrec] for r in range(nrec)]
    seqs = []
    for r in range(nrec):
        n = sum(len(infos[s.gid][0]) + gap for s in per[r]) + 64
        seq = background(rng, n)
        a = 32
        for s in per[r]:
            put(rng, seq, s, infos[s.gid][0], a)
            s.rec = r
            a += len(infos[s.gid][0]) + gap
        if dirty:
            seq[n - 8:n - 4] = b"NNNN"
        seqs.append(bytes(seq))
    return seqs, sites


# ---- scanning and checking --------------------------------------------------------------------------------------------

def hit_key(a):
    return np.lexsort((a["pos"], a["pattern"] & 0x7FFFFFFF, a["record"]))


def expected(cp, seqs, k, mode):
    parts = [synth_hits(cp, s, k, r, mode) for r, s in enumerate(seqs)]
    want = np.concatenate(parts) if parts else np.zeros(0, dtype=dist.HIT_DTYPE)
    return want[hit_key(want)]


def modes_differ(cp):
    return cp.scanned_patterns(0) != cp.scanned_patterns(1)


def scan_genome(cp, sc, seqs, fasta_path=None):
    g = engine.Genome(sum(len(s) for s in seqs) + 8192 * (len(seqs) + 2), max(len(seqs), 1))
    try:
        if fasta_path:
            with open(fasta_path, "w") as fh:
                for r, s in enumerate(seqs):
                    fh.write(">r%d\n" % r)
                    fh.write("\n".join(s[i:i + 60].decode("latin-1") for i in range(0, len(s), 60)) + "\n")
            assert g.add_fasta(fasta_path) == len(seqs)
        else:
            for r, s in enumerate(seqs):
                g.add_record("r%d" % r, s)
        assert [g.record_len(r) for r in range(len(seqs))] == [len(s) for s in seqs]
        _lib.check(_lib.lib().ipcr_scan_genome_hits(cp._h, sc._h, g._h))
        return dist.hits_from_scratch(sc), sc.stats()
    finally:
        g.close()


def compare(got, want, what):
    if len(got) == len(want) and all((got[f] == want[f]).all() for f in dist.HIT_DTYPE.names):
        return
    gs = set(map(tuple, got.tolist()))
    ws = set(map(tuple, want.tolist()))
    raise AssertionError("%s: %d hits, want %d; missing %s; extra %s" % (what, len(got), len(want), sorted(ws - gs)[:8], sorted(gs - ws)[:8]))


def check_sites(got, sites, infos, seqs, k, min_present, what):
    """the planted sites on their own, without the oracle: present ones at their position with exactly their planted
    index set (and reset flag), absent ones nowhere; the rule restated in site_idx must agree with the label"""
    have = {(int(h["record"]), int(h["pattern"]) & 0x7FFFFFFF, int(h["pos"])): (int(h["pattern"]) >> 31, int(h["mm0"]), int(h["mm1"]))
            for h in got}
    present = absent = 0
    for s in sites:
        pat, left, tw_dev, soff, slen = infos[s.gid]
        seq = seqs[s.rec]
        idx = site_idx(seq, s.pos, pat, left, tw_dev, k)
        assert (idx is not None) == s.present, (what, s.what, pat, s.subs)
        key = (s.rec, s.gid, s.pos)
        if s.present:
            m0 = sum(1 << j for j in idx if j < 64)
            m1 = sum(1 << (j - 64) for j in idx if j >= 64)
            flag = int(bool(slen) and any(ch not in b"ACGTacgt" for ch in seq[s.pos + soff:s.pos + soff + slen]))
            assert s.flag is None or s.flag == flag, (what, s.what)
            assert have.get(key) == (flag, m0, m1), (what, s.what, pat, sorted(s.subs), have.get(key), (flag, m0, m1))
            present += 1
        else:
            assert key not in have, (what, s.what, pat, sorted(s.subs))
            absent += 1
    assert present >= min_present, (what, present)
    return present, absent


TALLY = {}


def run_case(cp, sc, k, rng, want_kind, dirty, what, exhaustive_max_len=0, nrec=2, min_present=10, scan=None):
    mode = 1 if (dirty and modes_differ(cp)) else 0
    seqs, sites = records_with_sites(rng, cp, mode, k, dirty, exhaustive_max_len, nrec)
    infos = {g: cp.pattern_info(g) for g in cp.scanned_patterns(mode)}
    got, st = (scan or scan_genome)(cp, sc, seqs)
    assert st.kernel_kind == want_kind, (what, st.kernel_kind)
    assert st.segmented == 0 and st.pattern_set == mode, (what, st.segmented, st.pattern_set, mode)
    compare(got, expected(cp, seqs, k, st.pattern_set), what)
    pr, ab = check_sites(got, sites, infos, seqs, k, min_present, what)
    fam = {SPECIALISED: "specialised", TABLE: "table-driven", INDEX: "seed index"}[want_kind]
    t = TALLY.setdefault(fam, [0, 0])
    t[0] += pr
    t[1] += ab
    return got, st


def rand_primer(rng, L, iupac=0):
    s = [rng.choice("ACGT") for _ in range(L)]
    for _ in range(iupac):
        s[rng.randrange(L)] = rng.choice("RYSWKMBDHVN")
    return "".join(s)


# ---- the table-driven kernel: every instantiation ----------------------------------------------------------------------

@pytest.mark.parametrize("k", range(17))
def test_table_driven_every_counter_depth(k):
    """filter_generic_quad_kernel<K1 = k + 1, PB> for every k: PB = 4 / 2 / 1 patterns per walk, pattern counts that leave
    every residue of npat mod PB (the panel is cut with ipcr_panel_set_shard), lengths 8..128 mixed in one walk,
    terminal window 0 and 5, clean and dirty genomes (both pattern sets)"""
    rng = random.Random(7000 + k)
    pb = 4 if k <= 3 else (2 if k <= 7 else 1)
    lens = [L for L in (8, 12, 16, 20, 24, 31, 33, 40, 50, 64, 65, 100, 127, 128) if L >= 2 * k + 8]
    for tw, residue in ((5, k % pb), (0, (k + 1) % pb)):
        npat = pb * (2 if pb > 1 else 3) + residue
        # a shard of every c-th pattern (ids run F, R, rc F, rc R pair by pair: c = 3, 5, 7 mixes both window sides)
        npairs, c = next((n, c) for n in range(2, 40) for c in (3, 5, 7) if -(-4 * n // c) == npat)
        pairs = [P("p%d" % i, rand_primer(rng, lens[(2 * i) % len(lens)], i % 2), rand_primer(rng, lens[(2 * i + 1) % len(lens)]), 0, 0)
                 for i in range(npairs)]
        cfg = engine.Config(MaxMM=k, TerminalWindow=tw, MaxLen=500, HitCap=0, SeedLen=12 if k % 2 else 0)
        eng = engine.New(cfg)
        cp = eng.CompilePanel(pairs)
        cp.set_specialize(False)
        cp.set_shard(0, c)
        sc = eng.NewSimulationScratch(cp)
        for dirty in (False, True):
            mode = 1 if (dirty and modes_differ(cp)) else 0
            assert len(cp.scanned_patterns(mode)) == npat and npat % pb == residue
            assert len({len(cp.pattern_info(g)[0]) for g in cp.scanned_patterns(mode)}) >= 2      # mixed lengths in one walk
            run_case(cp, sc, k, rng, TABLE, dirty, "table k=%d tw=%d dirty=%d" % (k, tw, dirty),
                     exhaustive_max_len=24 if k <= 2 else (16 if k == 3 else 0), min_present=npat * 3)
        sc.close()
        cp.close()


# ---- the specialised filter --------------------------------------------------------------------------------------------

SPEC_K = (0, 1, 2, 3, 4, 8, 16)


def spec_panel(rng, k, long_):
    if long_:
        lens = (33, 40, 64, 65, 100, 128)
    else:
        lens = tuple(L for L in (16, 18, 20, 24, 28, 32) if L >= 2 * k) or (32,)
    return [P("p%d" % i, rand_primer(rng, lens[(2 * i) % len(lens)], i % 2), rand_primer(rng, lens[(2 * i + 1) % len(lens)]), 0, 0)
            for i in range(3)]


def spec_cases(k, long_, rng, what):
    tw = 3 if k % 2 == 0 else 5
    cfg = engine.Config(MaxMM=k, TerminalWindow=tw, MaxLen=500, HitCap=0, SeedLen=0 if k in (1, 8) else 12)
    eng = engine.New(cfg)
    cp = eng.CompilePanel(spec_panel(rng, k, long_))
    sc = eng.NewSimulationScratch(cp)
    for dirty in (False, True):
        _, st = run_case(cp, sc, k, rng, SPECIALISED, dirty, "%s k=%d dirty=%d" % (what, k, dirty),
                         exhaustive_max_len=(24 if k <= 2 else (16 if k == 3 else 0)) if not long_ else 0, min_present=12)
        if long_:
            assert st.verify_ms > 0, "primers beyond 32 nt: survivors go through the stand-alone verifier"
    sc.close()
    cp.close()


@pytest.mark.parametrize("long_", [False, True], ids=["le32", "33to128"])
@pytest.mark.parametrize("k", SPEC_K)
def test_specialised_filter(k, long_):
    """the panel-specialised filter: patterns of up to 32 nt verified inside the kernel, patterns of 33..128 nt filtered on
    the 20 positions next to their protected end and verified by verify_kernel"""
    spec_cases(k, long_, random.Random(8000 + 10 * k + long_), "specialised %s" % ("long" if long_ else "short"))


@pytest.mark.parametrize("k", (2, 8))
def test_specialised_filter_small_launches(k, monkeypatch):
    """the form in which four waves share a block (IPCR_JIT_SEGMENTS=4, read per launch): every launch here is small"""
    n_small = _lib.lib().ipcr_internal_small_launches
    n_small.restype = ctypes.c_uint64
    monkeypatch.setenv("IPCR_JIT_SEGMENTS", "4")
    before = n_small()
    for long_ in (False, True):
        spec_cases(k, long_, random.Random(8500 + 10 * k + long_), "segmented %s" % ("long" if long_ else "short"))
    assert n_small() >= before + 4


# ---- the seed index ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,knob", [(0, None), (1, None), (2, None), (3, None), (1, "IPCR_INDEX_FUSED"), (3, "IPCR_INDEX_FUSED"),
                                    (2, "IPCR_INDEX_SPLIT"), (3, "IPCR_INDEX_SPLIT"), (1, "IPCR_INDEX_HALF_BASES"), (3, "IPCR_INDEX_HALF_BASES"),
                                    (2, "long")])
def test_seed_index(k, knob, monkeypatch):
    """IPCR_FORCE_INDEX=1 (read per upload), the default fused form and each variant off (FUSED: per launch; SPLIT and
    HALF_BASES: when the panel's index is built); "long": primers > 32 nt in the panel, which the index cannot key -- its
    leftovers take spill-only specialised filters"""
    monkeypatch.setenv("IPCR_FORCE_INDEX", "1")
    if knob and knob != "long":
        monkeypatch.setenv(knob, "0")
    rng = random.Random(9000 + 10 * k + len(knob or ""))
    pairs = [P("p%d" % i, rand_primer(rng, rng.choice((16, 18, 20, 22, 24)), i % 3 == 1), rand_primer(rng, rng.choice((17, 20, 23))), 0, 0)
             for i in range(6)]
    if knob == "long":
        pairs += [P("l%d" % i, rand_primer(rng, 36 + 20 * i), rand_primer(rng, 40), 0, 0) for i in range(2)]
    tw = (3, 5, 0, 3)[k]
    cfg = engine.Config(MaxMM=k, TerminalWindow=tw, MaxLen=500, HitCap=0, SeedLen=12 if k != 2 else 0)
    eng = engine.New(cfg)
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    for dirty in (False, True):
        _, st = run_case(cp, sc, k, rng, INDEX, dirty, "index k=%d %s dirty=%d" % (k, knob, dirty),
                         exhaustive_max_len=(24 if k <= 2 else 16), min_present=40)
        if knob == "long":
            assert st.leftover_patterns >= 4 and st.leftover_kernels >= 1
    sc.close()
    cp.close()


# ---- the cold path: the first scan of a small panel before its kernels are built ----------------------------------------

COLD = r'''
import sys, random
sys.path[:0] = [%r, %r, %r]
import numpy as np
from ipcr_amd import engine
import test_gpu_hits as T
rng = random.Random(31)
cfg = engine.Config(MaxMM=2, TerminalWindow=5, MaxLen=500, HitCap=0, SeedLen=12)
eng = engine.New(cfg)
cp = eng.CompilePanel(T.spec_panel(rng, 2, False))
sc = eng.NewSimulationScratch(cp)
first, st1 = T.run_case(cp, sc, 2, random.Random(5), T.TABLE, True, "cold first scan", exhaustive_max_len=24)
cp.wait_ready()
later, st2 = T.run_case(cp, sc, 2, random.Random(5), T.SPECIALISED, True, "after the build", exhaustive_max_len=24)
T.compare(later, first, "cold vs built")
print("OK", st1.kernel_kind, st2.kernel_kind, len(first))
'''


def test_cold_small_panel_hits_equal_the_built_kernels(tmp_path):
    """IPCR_JIT_ASYNC=1 (read once per process: a child): the first scan of a small panel runs the table-driven kernel while
    hiprtc builds the specialised one; both give the same hit list, the exact one"""
    code = COLD % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    env = dict(os.environ, IPCR_JIT_ASYNC="1", IPCR_JIT_CACHE_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK 2 1"), (r.stdout, r.stderr[-3000:])


# ---- placement edges and loading paths ---------------------------------------------------------------------------------

def device_bar():
    how = _lib.lib().ipcr_internal_device_bar
    how.restype, how.argtypes = ctypes.c_int32, [ctypes.c_int32]
    return how(0)


EDGE_LENS = (0, 5, 4095, 4096, 4097, 262143, 262144, 262145, 4090, 30000)


def edge_records(rng, cp, k, modes, dirty):
    """records of the lengths where packing and tiling change (column 4096, block 262144), one shorter than the pattern and
    an empty one; in every record windows that start in strand rows 100..127 and windows across column and block ends
    (lane 63 reads the next block's column 0); by record (r % 3): 0 -- a site at position 0 and one that ends on the
    record's last base; 1 -- a site that overhangs the end by 1..k+1 bases (absent), 2 -- the rest of that site at its
    start (a site cut in two by the record boundary: absent).  `modes`: the pattern set each record is scanned with."""
    seqs, sites = [], []
    carry = b""
    for r, n in enumerate(EDGE_LENS):
        gids = cp.scanned_patterns(modes[r])
        infos = {g: cp.pattern_info(g) for g in gids}
        seq = background(rng, n)
        taken = []
        if carry and n > len(carry) + 64:
            seq[:len(carry)] = carry
            taken.append((0, len(carry)))
        carry = b""

        def free_at(pos, L):
            return 0 <= pos and pos + L <= n and not any(pos < e + 2 and b < pos + L + 2 for b, e in taken)

        def place(gid, pos, subs=None, what=""):
            L = len(infos[gid][0])
            if not free_at(pos, L):
                return
            s = Site(gid, subs or {}, True, what)
            put(rng, seq, s, infos[gid][0], pos)
            s.rec = r
            taken.append((pos, pos + L))
            sites.append(s)

        g0 = gids[r % len(gids)]
        L0 = len(infos[g0][0])
        if r % 3 == 0:
            place(g0, 0, what="at 0")
            alt = [ord(b) for b in "ACGT" if not MATCH[infos[g0][0][L0 // 2]][ord(b)]]
            place(g0, n - L0, {L0 // 2: alt[0]} if k and alt else None, what="ends on the last base")
        elif r % 3 == 1:
            over = 1 + (r // 3) % (k + 1)
            pos = n - L0 + over
            if free_at(pos, n - pos) and pos > 0:
                c = concrete(rng, infos[g0][0])
                seq[pos:n] = c[:n - pos]
                carry = bytes(c[n - pos:])
                taken.append((pos, n))
                s = Site(g0, {}, False, "overhangs by %d" % over)
                s.rec, s.pos = r, pos
                sites.append(s)
        if dirty and n:                                    # a reset byte in every non-empty record
            q = next((q for q in (2000, 1000, 2, 0) if free_at(q, 1)), None)
            if q is not None:
                seq[q] = ord("N")
                taken.append((q, q + 1))
        for g in gids:
            for base in (0, 4096, 8192 * 3, 131072, 258048):
                for row in (100, 109, 118, 125, 127):
                    place(g, base + row + 128 * rng.randrange(32), what="row %d" % row)
            for end in (4096, 8192, 262144):
                L = len(infos[g][0])
                for d in (1, L // 2, L - 1):
                    place(g, end - d, what="across %d" % end)
        seqs.append(bytes(seq))
    return seqs, sites


def edge_case(cp, k, dirty, scan, modes, what):
    """scan the edge records (`modes`: the pattern set each record must be scanned with) and check the list"""
    rng = random.Random(1234 + k + dirty)
    seqs, sites = edge_records(rng, cp, k, modes, dirty)
    got, sts = scan(seqs)
    for st in sts:
        assert st.segmented == 0
    seen = [st.pattern_set for st in sts] if len(sts) == len(seqs) else [sts[0].pattern_set] * len(seqs)
    assert seen == modes, (what, seen, modes)
    parts = [synth_hits(cp, s, k, r, modes[r]) for r, s in enumerate(seqs)]
    want = np.concatenate(parts)
    compare(got, want[hit_key(want)], what)
    present = absent = 0
    for m in set(modes):
        infos = {g: cp.pattern_info(g) for g in cp.scanned_patterns(m)}
        pr, ab = check_sites(got, [s for s in sites if modes[s.rec] == m], infos, seqs, k, 0, what)
        present, absent = present + pr, absent + ab
    assert present >= 100, (what, present)
    t = TALLY.setdefault("placement edges and loading paths", [0, 0])
    t[0] += present
    t[1] += absent
    return got


def genome_scan(cp, sc, fasta=None):
    def run(seqs):
        got, st = scan_genome(cp, sc, seqs, fasta)
        return got, [st]
    return run


def chunk_scan(eng, cp, sc, env, monkeypatch):
    """every record through ipcr_scan_chunk on one scratch; `env` per call (a list: toggled between calls); the hits of
    call r renumbered to record r"""
    def run(seqs):
        parts, sts = [], []
        for r, s in enumerate(seqs):
            for name, val in env[r % len(env)].items():
                monkeypatch.setenv(name, val)
            eng.SimulateCompiledWithScratch("r%d" % r, s, cp, sc)
            h = dist.hits_from_scratch(sc)
            assert (h["record"] == 0).all()
            h["record"] = r
            parts.append(h)
            sts.append(sc.stats())
        return np.concatenate(parts), sts
    return run


@pytest.fixture(scope="module")
def edge_panels():
    """one panel per kernel, reused by every loading path (ipcr_panel_set_specialize holds from the panel's first scan on)"""
    cfg = engine.Config(MaxMM=2, TerminalWindow=3, MaxLen=500, HitCap=0, SeedLen=0)
    eng = engine.New(cfg)
    cps = {}
    for kernel in ("specialised", "table"):
        cps[kernel] = eng.CompilePanel([P("a", "ACGTTGCATGGATCCTAACG", "AGAGTTTGATCMTGGCTCAGTTAC", 0, 0)])
        cps[kernel].set_specialize(kernel == "specialised")
    yield cfg, eng, cps
    for cp in cps.values():
        cp.close()


@pytest.mark.parametrize("kernel", ["specialised", "table"])
@pytest.mark.parametrize("path", ["genome", "genome_no_bar", "fasta", "chunk_ascii", "chunk_hostpack_bar", "chunk_hostpack_dma", "chunk_toggle"])
def test_loading_paths_and_placement_edges(edge_panels, kernel, path, monkeypatch, tmp_path):
    """the same records give the same hit list (records renumbered) through Genome.add_record (the device packs records below
    4096 bases; from 4096 on the host packs them through the BAR; IPCR_CHUNK_BAR=0: the device packs all), a FASTA file, and
    ipcr_scan_chunk with IPCR_CHUNK_HOSTPACK 0/1 x IPCR_CHUNK_BAR 0/1 (and toggled between calls on one scratch); the
    records interleave host-packed and ASCII loads (4096, 4090, 4096 bases ... in one genome), the case that once left a
    re-allocated staging buffer marked fine-grained"""
    cfg, eng, cps = edge_panels
    cp = cps[kernel]
    bar = device_bar()
    if path in ("genome", "chunk_hostpack_bar", "chunk_toggle") and bar == 0:
        pytest.skip("no large BAR on this device: the host packer does not write through it, the path does not exist here")
    sc = eng.NewSimulationScratch(cp)
    want_kind = SPECIALISED if kernel == "specialised" else TABLE
    if path == "genome":
        monkeypatch.setenv("IPCR_CHUNK_BAR", "1")
        scan = genome_scan(cp, sc)
    elif path == "genome_no_bar":
        monkeypatch.setenv("IPCR_CHUNK_BAR", "0")
        scan = genome_scan(cp, sc)
    elif path == "fasta":
        scan = genome_scan(cp, sc, str(tmp_path / "edges.fa"))
    elif path == "chunk_ascii":
        scan = chunk_scan(eng, cp, sc, [{"IPCR_CHUNK_HOSTPACK": "0", "IPCR_CHUNK_BAR": "1"}], monkeypatch)
    elif path == "chunk_hostpack_bar":
        scan = chunk_scan(eng, cp, sc, [{"IPCR_CHUNK_HOSTPACK": "1", "IPCR_CHUNK_BAR": "1"}], monkeypatch)
    elif path == "chunk_hostpack_dma":
        scan = chunk_scan(eng, cp, sc, [{"IPCR_CHUNK_HOSTPACK": "1", "IPCR_CHUNK_BAR": "0"}], monkeypatch)
    else:
        scan = chunk_scan(eng, cp, sc, [{"IPCR_CHUNK_HOSTPACK": "1", "IPCR_CHUNK_BAR": "1"}, {"IPCR_CHUNK_HOSTPACK": "0", "IPCR_CHUNK_BAR": "1"}], monkeypatch)
    differ = modes_differ(cp)
    for dirty in (False, True):
        # the pattern set of each record: a genome takes the raw set when any record holds a reset byte; a chunk the host
        # packs knows whether it holds one, a chunk the device packs takes the raw set whatever it holds
        modes = []
        for r, n in enumerate(EDGE_LENS):
            if path.startswith("chunk"):
                hostpacked = path in ("chunk_hostpack_bar", "chunk_hostpack_dma") or (path == "chunk_toggle" and r % 2 == 0)
                modes.append(1 if differ and ((dirty and n > 0) or not hostpacked) else 0)
            else:
                modes.append(1 if differ and dirty else 0)
        edge_case(cp, 2, dirty, scan, modes, "%s %s dirty=%d" % (kernel, path, dirty))
        assert sc.stats().kernel_kind == want_kind
    sc.close()


def test_interleaved_host_packed_and_ascii_records(edge_panels, monkeypatch):
    """one Genome: 4096 bases (host-packed through the BAR), 4090 (ASCII: the staging buffer re-allocated with plain
    hipMalloc), 4096 again (host-packed: must re-allocate fine-grained memory before it writes through the BAR), then a
    larger record; sites in every record, the exact hit list"""
    if device_bar() == 0:
        pytest.skip("no large BAR on this device: every record is packed on the device")
    cfg, eng, cps = edge_panels
    cp = cps["specialised"]
    monkeypatch.setenv("IPCR_CHUNK_BAR", "1")
    sc = eng.NewSimulationScratch(cp)
    rng = random.Random(77)
    gids = cp.scanned_patterns(0)
    infos = {g: cp.pattern_info(g) for g in gids}
    seqs, sites = [], []
    for r, n in enumerate((4096, 4090, 4096, 300_000, 4090, 8192)):
        seq = background(rng, n)
        a = 3
        while a + 40 < n and a < 20000:
            g = gids[a % len(gids)]
            s = Site(g, {}, True, "rec %d" % r)
            put(rng, seq, s, infos[g][0], a)
            s.rec = r
            sites.append(s)
            a += 97
        seqs.append(bytes(seq))
    got, st = scan_genome(cp, sc, seqs)
    assert st.pattern_set == 0 and st.kernel_kind == SPECIALISED
    compare(got, expected(cp, seqs, 2, 0), "interleaved")
    check_sites(got, sites, infos, seqs, 2, 300, "interleaved")
    sc.close()


def test_tally_of_checked_sites():
    """(runs last in this file: the number of planted sites checked per kernel family, printed for the record)"""
    for fam, (pr, ab) in sorted(TALLY.items()):
        print("%s: %d present, %d absent sites checked" % (fam, pr, ab))
    assert not TALLY or all(pr > 0 for pr, _ in TALLY.values())
