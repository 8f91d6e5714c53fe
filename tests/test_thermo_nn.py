"""ipcr-thermo, --thermo-model nn-duplex-v1, without a device: thermo.PerfectDuplex and ipcr_thermo_nn_duplex_end against the
reference's recorded rows (tests/golden/thermo, tests/golden/thermo_nn) and, bit for bit, against tests/nn_restatement.py;
the refusals; the ABI names.

The per-term clamp `w < 0` of the model cannot be reached with the tables as they stand -- every ddG is at least 0.60, the N
heuristic at least 0.95, the weights and the terminal term are positive -- so no case is made up for it."""
import ctypes as C
import math
import os
import random
import re
import struct

import pytest

import nn_restatement as NN
import thermo_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIP = R.load_triplets()
DANG = NN.load_dangling()


def cond_of(r):
    from ipcr_amd import thermo
    return thermo.Conditions(AnnealC=float(r["anneal_c"]), NaM=float(r["na_m"]), MgM=float(r["mg_m"]), DntpM=float(r["dntp_m"]),
                             PrimerTotalM=float(r.get("primer_total_m") or 0), SaltModel=thermo.ParseSaltModel(r["salt_model"]))


def base_of(primer, cond):
    """(tm_c, denom) as ImperfectDuplex takes them from PerfectDuplex (imperfect.go:268-276)"""
    from ipcr_amd import thermo
    d = thermo.PerfectDuplex(primer, cond)
    return d.TmC, abs(d.EffectiveDenomCalK)


@pytest.mark.parametrize("name", ["perfect_duplex_goldens.golden", "salt_goldens.golden"])
def test_perfect_duplex_reproduces_the_fixture_rows(name):
    from ipcr_amd import thermo
    rows = R.golden_rows(name)
    assert rows
    for r in rows:
        assert r["target3to5"] == "".join(R.COMP[c] for c in r["seq"])  # the rows are primers on their own complements
        d = thermo.PerfectDuplex(r["seq"], cond_of(r))
        tol = float(r["tolerance"])
        assert abs(d.TmC - float(r["tm_c"])) <= tol, (r["id"], d.TmC)
        assert abs(d.AnnealMarginC - float(r["margin_c"])) <= tol, (r["id"], d.AnnealMarginC)
        assert abs(d.DeltaGAtAnnealKcal - float(r["dg_kcal"])) <= tol, (r["id"], d.DeltaGAtAnnealKcal)
        assert d.EffectiveDenomCalK < 0 and d.AnnealC == float(r["anneal_c"])
    with pytest.raises(ValueError):
        thermo.PerfectDuplex("ACGRT", thermo.DefaultConditions())
    with pytest.raises(ValueError):
        thermo.PerfectDuplex("", thermo.DefaultConditions())


def test_mismatch_rows():
    """mismatch_goldens.golden: tm_c, mismatch_penalty_c and mismatch_count at the row's tolerance"""
    from ipcr_amd import thermo
    rows = NN.golden_rows("mismatch_goldens.golden")
    assert rows
    for r in rows:
        tm, D = base_of(r["primer"], cond_of(r))
        e = thermo.nn_duplex_end(r["primer"], r["target3to5"], "", tm, D)
        tol = float(r["tolerance"])
        assert e.status == 0
        assert abs(e.tm_c - float(r["tm_c"])) <= tol, (r["id"], e.tm_c)
        assert abs(e.mismatch_penalty_c - float(r["mismatch_penalty_c"])) <= tol, (r["id"], e.mismatch_penalty_c)
        assert abs(e.mismatch_penalty_c * D / 1000.0 - float(r["dg_penalty_kcal"])) <= tol
        assert e.mismatch_count == int(r["mismatch_count"])
        assert e.dangling_adjustment_c == 0.0 and e.n_count == 0


def test_triplet_rows():
    """the 192 rows of mismatch_triplet_goldens.golden: one mismatch in the middle of a 7-mer, weight 1.0, no terminal term"""
    from ipcr_amd import thermo
    rows = R.golden_rows("mismatch_triplet_goldens.golden")
    assert len(rows) == 192
    for r in rows:
        tm, D = base_of(r["primer"], cond_of(r))
        e = thermo.nn_duplex_end(r["primer"], r["target"], "", tm, D)
        assert e.status == 0 and e.mismatch_count == int(r["expected_mismatch_count"]) == 1
        got = e.mismatch_penalty_c * D / 1000.0
        assert abs(got - float(r["expected_delta_delta_g_kcal"])) <= float(r["tolerance_delta_g"]), (r["id"], got)
        assert e.tm_c < tm                                              # expected_tm_direction: decrease
        assert r["expected_tm_direction"] == "decrease"


def test_dangling_context_rows():
    """The rows of dangling_end_context_goldens.golden that give only three_prime_base (the file holds two: the other three
    give a five_prime_base, which the product score never passes): -(dangling_adjustment_c) * denom / 1000 against
    expected_delta_g_kcal at 1e-9, the tolerance of the reference's other derived columns -- the file's own 1e-12 is for the
    table value, and the round trip through denom costs a few ulp.  Measured differences: threeprime_target5p_GA_T 0.0,
    threeprime_target5p_GT_A_unfavorable 0.0 (the round trip happened to be exact for both)."""
    from ipcr_amd import thermo
    rows = [r for r in NN.golden_rows("dangling_end_context_goldens.golden") if r["three_prime_base"] and not r["five_prime_base"]]
    assert len(rows) == 2
    for r in rows:
        tm, D = base_of(r["primer"], cond_of(r))
        e = thermo.nn_duplex_end(r["primer"], r["target3to5"], r["three_prime_base"], tm, D)
        got = -e.dangling_adjustment_c * D / 1000.0
        print(r["id"], "difference", abs(got - float(r["expected_delta_g_kcal"])))
        assert abs(got - float(r["expected_delta_g_kcal"])) <= 1e-9, (r["id"], got)
        assert e.status == 0 and e.mismatch_count == 0 and e.mismatch_penalty_c == 0.0
        assert (e.tm_c > tm) == (r["expected_tm_direction"] == "increase") and e.tm_c != tm
        assert int(r["expected_dangling_count"]) == 1
    # the sixteen keys: each value of the fixture's 5p rows comes back through the entry point
    for (x, paired), g in DANG.items():
        P = "ACGTACGTACGTACG" + R.COMP[paired]
        T = "".join(R.COMP[c] for c in P)
        e = thermo.nn_duplex_end(P, T, x, 50.0, 250.0)
        assert abs(-e.dangling_adjustment_c * 250.0 / 1000.0 - g) <= 1e-9, (x, paired)


def bits(e):
    return (struct.pack("<3d", e.tm_c, e.mismatch_penalty_c, e.dangling_adjustment_c), e.mismatch_count, e.n_count, e.status)


def random_case(rng):
    n = rng.choice((1, 2, 3, 4, 5, 6, 7, 127, 128)) if rng.random() < 0.3 else rng.randint(1, 128)
    P = "".join(rng.choice("ACGT") for _ in range(n))
    T = [R.COMP[c] for c in P]
    k = rng.randint(0, 4)
    where = set()
    if k and rng.random() < 0.5:                                        # a run of adjacent columns
        a = rng.randrange(n)
        where |= {min(n - 1, a + j) for j in range(k)}
    else:
        where |= {rng.randrange(n) for _ in range(k)}
    if k and rng.random() < 0.4:
        where |= {rng.choice((0, n - 1))}
    if k and rng.random() < 0.15:
        where |= {0, n - 1}
    for i in where:
        T[i] = rng.choice([c for c in "ACGTN" if c != T[i]])
    T = "".join(T)
    if rng.random() < 0.2:
        P, T = P.lower(), "".join(c.lower() if rng.random() < 0.5 else c for c in T)
    dangling = rng.choice(["A", "C", "G", "T", "N", "", "a", "g"])
    return P, T, dangling, rng.uniform(20.0, 90.0), rng.uniform(80.0, 700.0)


def test_bit_for_bit_against_the_restatement():
    from ipcr_amd import thermo
    rng = random.Random(20240)
    seen_mm, seen_len, seen_d, adj, terminal = set(), set(), set(), 0, 0
    for _ in range(2000):
        P, T, x, tm, D = random_case(rng)
        got = thermo.nn_duplex_end(P, T, x, tm, D)
        want = NN.end(P, T, x, tm, D, TRIP, DANG)
        assert bits(got) == want.key(), (P, T, x, tm, D, got.tm_c, want.tm_c)
        seen_mm.add(want.mm)
        seen_len.add(len(P))
        seen_d.add(x.upper())
        adj += want.adj != 0.0
        terminal += NN._read(T[-1]) != R.COMP[P[-1].upper()] or NN._read(T[0]) != R.COMP[P[0].upper()]
    assert seen_mm >= {0, 1, 2, 3, 4} and {1, 2, 128} <= seen_len and seen_d == {"A", "C", "G", "T", "N", ""}
    assert adj > 300 and terminal > 300
    # n == 1: the 3' test comes first
    e = thermo.nn_duplex_end("A", "A", "", 50.0, 200.0)
    assert bits(e) == NN.end("A", "A", "", 50.0, 200.0, TRIP, DANG).key()
    assert e.mismatch_penalty_c == (1.40 * 1000.0) / 200.0 * 2.0 + 1.5
    # a target byte outside ACGTN reads as N: the one deviation
    assert bits(thermo.nn_duplex_end("ACGT", "TGRA", "", 50.0, 200.0)) == bits(thermo.nn_duplex_end("ACGT", "TGNA", "", 50.0, 200.0))
    assert thermo.nn_duplex_end("ACGT", "TGNA", "", 50.0, 200.0).n_count == 1


def test_refusals_of_the_end_call():
    from ipcr_amd import _lib, thermo
    L = _lib.lib()
    out = _lib.ThermoNNEnd()

    def status(*a):
        return L.ipcr_thermo_nn_duplex_end(*a, C.byref(out))
    assert status(b"ACGT", b"TGCA", b"\0", 50.0, 200.0) == _lib.OK and out.status == 0
    assert status(b"ACGT", b"TGC", b"\0", 50.0, 200.0) == _lib.ERR_INVALID
    assert "length" in L.ipcr_last_error().decode()
    assert status(b"", b"", b"\0", 50.0, 200.0) == _lib.ERR_INVALID
    assert status(b"A" * 129, b"T" * 129, b"\0", 50.0, 200.0) == _lib.ERR_INVALID
    for tm, D in ((50.0, 0.0), (50.0, -200.0), (50.0, math.nan), (50.0, math.inf), (math.nan, 200.0), (math.inf, 200.0)):
        assert status(b"ACGT", b"TGCA", b"\0", tm, D) == _lib.ERR_INVALID, (tm, D)
    assert L.ipcr_thermo_nn_duplex_end(None, b"TGCA", b"\0", 50.0, 200.0, C.byref(out)) == _lib.ERR_INVALID
    assert L.ipcr_thermo_nn_duplex_end(b"ACGT", b"TGCA", b"\0", 50.0, 200.0, None) == _lib.ERR_INVALID
    # a primer byte outside ACGT: not an error of the call, status 1 and NaN
    e = thermo.nn_duplex_end("ACRT", "TGCA", "G", 50.0, 200.0)
    assert e.status == 1 and math.isnan(e.tm_c) and e.mismatch_count == 0
    assert thermo.nn_duplex_end("ACNT", "TGCA", "", 50.0, 200.0).status == 1


def test_base_table_refusals_need_no_device():
    """n_base and the base entries are checked against the scratch's panel before anything else: a host-only scratch shows it"""
    from ipcr_amd import _lib, engine, primer, thermo
    L = _lib.lib()
    eng = engine.New(engine.Config(MaxMM=1))
    pairs = [primer.Pair("a", "ACGTACGTACGTACGTAC", "TTGACCATGACCATGACC"), primer.Pair("b", "ACGRACGTACGTACGTAC", "TTGACCATGACCATGAAA")]
    cp = eng.CompilePanel(pairs)
    sc = engine.SimulationScratch(cp, host_only=True)
    base = thermo.panel_nn_base(pairs, thermo.DefaultConditions())
    assert len(base) == 4 and all(math.isfinite(t) and math.isfinite(d) and d > 0 for t, d in base)
    assert base[0] == base_of(pairs[0].Forward, thermo.score_conditions(thermo.DefaultConditions()))
    assert base[2][1] == 200.0                                          # the IUPAC primer's placeholder
    out = (C.c_double * 1)()

    def status(entries, n_base=None, anneal=60.0):
        b = (_lib.ThermoNNPrimer * max(len(entries), 1))(*(_lib.ThermoNNPrimer(t, d) for t, d in entries))
        return L.ipcr_thermo_nn_duplex_scratch_products(sc._h, b, len(entries) if n_base is None else n_base, anneal, out, None, 0)
    assert status(base) == _lib.ERR_DEVICE                              # a good table gets as far as "host-only scratch"
    assert status(base[:3]) == _lib.ERR_INVALID and "n_base" in L.ipcr_last_error().decode()
    assert status(base, 2) == _lib.ERR_INVALID
    assert status(base + base) == _lib.ERR_INVALID
    assert L.ipcr_thermo_nn_duplex_scratch_products(sc._h, None, 4, 60.0, out, None, 0) == _lib.ERR_INVALID
    for bad in ((50.0, 0.0), (50.0, -1.0), (50.0, math.nan), (50.0, math.inf), (math.nan, 200.0), (-math.inf, 200.0)):
        assert status(base[:3] + [bad]) == _lib.ERR_INVALID, bad
        assert "base entry 3" in L.ipcr_last_error().decode()
    assert status(base, anneal=math.nan) == _lib.ERR_INVALID
    assert L.ipcr_thermo_nn_duplex_scratch_products(None, None, 0, 60.0, out, None, 0) == _lib.ERR_INVALID
    assert L.ipcr_thermo_nn_duplex_products(sc._h, None, None, 0, 60.0, out, None, 0) == _lib.ERR_INVALID
    sc.close()
    cp.close()


def test_abi_declares_the_nn_entry_points():
    from ipcr_amd import _lib, thermo
    h = open(os.path.join(ROOT, "include", "ipcr_hip.h")).read()
    for name in ("ipcr_thermo_nn_duplex_products", "ipcr_thermo_nn_duplex_scratch_products", "ipcr_thermo_nn_duplex_end"):
        assert re.search(r"\bipcr_status\s+%s\s*\(" % name, h), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert re.search(r"typedef struct ipcr_thermo_nn_primer \{", h) and re.search(r"typedef struct ipcr_thermo_nn_end \{", h)
    assert C.sizeof(_lib.ThermoNNEnd) == 32 and C.sizeof(_lib.ThermoNNPrimer) == 16
    assert "#define IPCR_ABI_VERSION 6" in h                            # additive: the version stays
    assert "nn-duplex-v1" in thermo.UNBUILT_MODELS                      # the driver still refuses the model
