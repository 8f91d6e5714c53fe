"""ipcr-thermo, --thermo-model legacy-heuristic, without a device: the host entry points (the arithmetic the kernel runs:
thermo_legacy.h) against the fixture tables and a restatement written in tests/thermo_restatement.py, the perfect-duplex Tm
behind --denom auto, Go's float formats, the score ordering, panel construction and every refusal of the driver."""
import io
import json
import math
import os
import random
import struct

import pytest

import thermo_restatement as R
from ipcr_amd import _lib, engine, primer, thermo, thermo_cli

TRIP = R.load_triplets()
LIT = json.load(open(os.path.join(R.GOLDEN, "literals.json")))
AUTO_D = thermo.denom_for_primer("GGAAAGACATATCCCAATACAGCAA", thermo.DefaultConditions())


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


# ---------------------------------------------------------------- the look-up

def test_triplet_fixture_shape():
    rows = R.golden_rows("mismatch_triplet_goldens.golden")
    assert len(rows) == 192 and len(TRIP) == 192
    for r in rows:
        p, t = r["primer"], r["target"]
        assert len(p) == 7 and len(t) == 7
        assert [i for i in range(7) if R.COMP[p[i]] != t[i]] == [3]
        assert r["expected_triplet_count"] == "1" and float(r["tolerance_delta_g"]) == 1e-9


def test_mismatch_ddg_equals_every_fixture_row():
    for r in R.golden_rows("mismatch_triplet_goldens.golden"):
        p, t = r["primer"], r["target"]
        got = thermo.mismatch_ddg(p[2], p[3], p[4], t[2], t[3], t[4])
        assert abs(got - float(r["expected_delta_delta_g_kcal"])) <= float(r["tolerance_delta_g"]), (r["id"], got)


def test_mismatch_ddg_pair_family_and_n_branches():
    """every (flank, centre) combination over ACGTN: the triplet where it applies, the pair family where a flank does not
    pair or is N, the heuristic for t == N; and the bytes the reference's look-up refuses"""
    S = "ACGTN"
    seen = {"triplet": 0, "pair": 0, "n": 0}
    for p5 in S:
        for p in "ACGT":
            for p3 in S:
                for t5 in S:
                    for t in S:
                        for t3 in S:
                            want = R.ddg(p5, p, p3, t5, t, t3, TRIP)
                            got = thermo.mismatch_ddg(p5, p, p3, t5, t, t3)
                            assert bits(got) == bits(want), (p5, p, p3, t5, t, t3, got, want)
                            seen["n" if t == "N" else "triplet" if (p5, p, p3, t5, t, t3) in TRIP else "pair"] += 1
    assert seen["triplet"] == 192 and seen["pair"] > 0 and seen["n"] > 0
    assert thermo.mismatch_ddg("G", "A", "C", "G", "N", "C") == 1.0 - 0.05      # four G/C flanks
    assert thermo.mismatch_ddg("G", "A", "C", "A", "N", "N") == 1.0             # two G/C against one A/T: not two more
    assert thermo.mismatch_ddg("G", "A", "C", "N", "N", "N") == 1.0 - 0.05      # two G/C, no A/T
    assert thermo.mismatch_ddg("x", "A", "-", "a", "N", "g") == 1.0             # flanks outside ACGT count as neither
    assert thermo.mismatch_ddg("a", "A", "c", "T", "C", "G") == R.PAIR[("A", "C")]  # lower-case flanks are N: no triplet
    for p, t in (("N", "A"), ("a", "T"), ("R", "N"), ("A", "n"), ("A", "R"), ("A", "-"), ("\x00", "A")):
        with pytest.raises(_lib.IpcrError) as e:
            thermo.mismatch_ddg("A", p, "A", "T", t, "T")
        assert e.value.status == _lib.ERR_INVALID


# ---------------------------------------------------------------- the penalty

def _random_pair(rng, n):
    P = "".join(rng.choice("ACGT") for _ in range(n))
    T = []
    for ch in P:
        u = rng.random()
        T.append(R.COMP[ch] if u < 0.6 else "N" if u < 0.7 else rng.choice("ACGT"))
    return P, "".join(T)


@pytest.mark.parametrize("denom", [200.0, AUTO_D, 0.0, -35.5])
def test_penalty_equals_the_restatement_bit_for_bit(denom):
    rng = random.Random(20260117)
    lengths = list(range(1, 129)) + [rng.randint(1, 128) for _ in range(400)]
    some_mismatch = 0
    for n in lengths:
        P, T = _random_pair(rng, n)
        got, want = thermo.legacy_penalty(P, T, denom), R.closed_form(P, T, denom, TRIP)
        assert bits(got) == bits(want), (n, P, T, denom, got, want)
        some_mismatch += want > 0
    assert some_mismatch > 300
    assert AUTO_D > 0 and AUTO_D != 200.0 and math.isfinite(AUTO_D)


def test_penalty_edge_strings():
    assert bits(thermo.legacy_penalty("ACGT", "TGCA")) == bits(0.0)                # perfect: +0.0
    assert thermo.legacy_penalty("ACGR", "TGCA") == 0.0                            # primer not pure ACGT
    assert thermo.legacy_penalty("ACGT", "TGC-") == 0.0                            # target outside ACGTN
    assert thermo.legacy_penalty("", "TGCA") == 0.0 and thermo.legacy_penalty("ACGT", "") == 0.0
    assert bits(thermo.legacy_penalty("aagtac", "tgcatg")) == bits(thermo.legacy_penalty("AAGTAC", "TGCATG"))
    assert bits(thermo.legacy_penalty("AAGTAC", "TGCATG")) == bits(18.975)
    assert bits(thermo.legacy_penalty("AAGTAC", "TCCATG")) == bits(29.625)
    with pytest.raises(_lib.IpcrError) as e:
        thermo.legacy_penalty("ACGT", "TGCAT")
    assert e.value.status == _lib.ERR_INVALID
    # denom <= 0: every mismatch costs 4.0 times its weight
    assert thermo.legacy_penalty("AAAAAAAAAA", "TTTTATTTTT", 0.0) == 4.0
    assert thermo.legacy_penalty("AAAAAAAAAA", "ATTTTTTTTA", -1.0) == 4.0 * 1.5 + 4.0 * 2.0


@pytest.mark.parametrize("allow_gap", [False, True])
def test_gap_dp_equals_the_closed_form(allow_gap):
    """the reference's DP, literally, with and without its one 1-nt gap: for |P| == |T| the gap state never reaches the
    last cell, so --allow-indel cannot change a legacy-heuristic score"""
    rng = random.Random(7)
    for k in range(300):
        n = rng.randint(1, 40) if k else 128
        P, T = _random_pair(rng, n)
        for D in (200.0, AUTO_D, 0.0):
            a, b = R.gap_dp(P, T, D, allow_gap, TRIP), R.closed_form(P, T, D, TRIP)
            assert bits(a) == bits(b), (P, T, D, a, b)
    # many mismatches, where a gap would be cheap if it could be used
    P = "ACGTACGTACGTACGTACGT"
    T = R.comp_window(P[1:].encode() + b"A")
    assert bits(R.gap_dp(P, T, 200.0, True, TRIP)) == bits(R.closed_form(P, T, 200.0, TRIP)) == bits(thermo.legacy_penalty(P, T))


def test_position_effects():
    """TestAlignPenalty_PositionEffects (score_test.go:19-61)"""
    pr, perfect = "ACGTACGTAC", "TGCATGCATG"
    assert thermo.legacy_penalty(pr, perfect) == 0
    t3 = perfect[:-1] + ("G" if perfect[-1] == "A" else "A")
    t5 = ("A" if perfect[0] == "T" else "T") + perfect[1:]
    ti = perfect[:4] + ("G" if perfect[4] == "A" else "A") + perfect[5:]
    p3, p5, pin = (thermo.legacy_penalty(pr, t) for t in (t3, t5, ti))
    assert p3 > p5 and pin > 0


# ---------------------------------------------------------------- conditions, Tm, denominators

@pytest.mark.parametrize("name", ["perfect_duplex_goldens.golden", "salt_goldens.golden"])
def test_tm_reproduces_the_fixture_rows(name):
    rows = R.golden_rows(name)
    assert rows
    models = set()
    for r in rows:
        p = r["seq"]
        cond = thermo.Conditions(AnnealC=float(r["anneal_c"]), NaM=float(r["na_m"]), MgM=float(r["mg_m"]), DntpM=float(r["dntp_m"]),
                                 PrimerTotalM=float(r["primer_total_m"]), SaltModel=thermo.ParseSaltModel(r["salt_model"]),
                                 SelfComplementary=p == "".join(R.COMP[c] for c in reversed(p)))   # as PerfectDuplex sets it
        res = thermo.Tm(p, r["target3to5"], cond.TmInput())
        assert abs(res.TmC - float(r["tm_c"])) <= float(r["tolerance"]), (r["id"], res.TmC)
        if "effective_na_m" in r:
            assert abs(cond.EffectiveNaM() - float(r["effective_na_m"])) <= 1e-9
            assert abs(cond.FreeMgM() - float(r["free_mg_m"])) <= 1e-9
        models.add(r["salt_model"])
    if name.startswith("salt"):
        assert models == {"monovalent", "owczarzy-lite", "owczarzy08"}


def test_concentration_and_salt_literals():
    for c in LIT["conc"]:
        assert abs(thermo.ParseConc(c["text"]) - c["mol_per_l"]) <= c["abs_tol"]
    assert thermo.ParseConc("50mM") == 50 * 1e-3 and thermo.ParseConc("250nM") == 250 * 1e-9 and thermo.ParseConc("1M") == 1.0
    assert thermo.ParseConc(" 3 uM ") == 3 * 1e-6
    for bad in ("", "abc", "5", "5xM", "-1mM"):
        with pytest.raises(ValueError):
            thermo.ParseConc(bad)
    for m in LIT["salt_models"]:
        assert thermo.ParseSaltModel(m) == (m or "monovalent")
    for m in LIT["salt_models_rejected"]:
        with pytest.raises(ValueError):
            thermo.ParseSaltModel(m)
    e = LIT["effective_monovalent"]
    assert thermo.EffectiveMonovalent(e["na_m"], e["mg_m"], 0, "monovalent") == e["na_m"]
    assert thermo.EffectiveMonovalent(e["na_m"], e["mg_m"], 0, "owczarzy-lite") > e["na_m"]
    t = LIT["tm_input"]
    c = thermo.Conditions(AnnealC=t["anneal_c"], NaM=t["na_m"], MgM=t["mg_m"], PrimerTotalM=t["primer_total_m"],
                          SaltModel=t["salt_model"], SelfComplementary=t["self_complementary"])
    inp = c.TmInput()
    assert inp.CT == c.PrimerTotalM and inp.X == 1 and inp.Na > c.NaM
    for f in LIT["free_mg"]:
        got = thermo.FreeMagnesium(f["mg_m"], f["dntp_m"])
        assert got < f["below"] and (got > f["above"] if "above" in f else got >= f["at_least"])
    w = LIT["owczarzy08_input"]
    c = thermo.Conditions(NaM=w["na_m"], MgM=w["mg_m"], DntpM=w["dntp_m"], PrimerTotalM=w["primer_total_m"], SaltModel="owczarzy08")
    inp = c.TmInput()
    assert (inp.SaltModel, inp.Na, inp.Mg, inp.Dntp) == ("owczarzy08", c.NaM, c.MgM, c.DntpM)
    assert 0.002 < c.FreeMgM() < c.MgM


def test_denominator_is_a_property_of_the_primer():
    d = thermo.DefaultConditions()
    a = thermo.denom_for_primer("AAGTAC", d)
    assert a > 0 and a != 200.0
    assert thermo.denom_for_primer("aagtac", d) == a
    assert thermo.denom_for_primer("AAGTRC", d) == 200.0 and thermo.denom_for_primer("", d) == 200.0
    # self-complementary: X = 1 and the symmetry term
    assert thermo.denom_for_primer("GGTACC", d) != thermo.denom_for_primer("GGTACG", d)
    lo = thermo.Conditions(AnnealC=60, NaM=0.01, MgM=0.003, PrimerTotalM=1e-7, SaltModel="monovalent")
    hi = thermo.Conditions(AnnealC=60, NaM=0.2, MgM=0.003, PrimerTotalM=1e-6, SaltModel="monovalent")
    assert thermo.denom_for_primer("AAGTAC", lo) != thermo.denom_for_primer("AAGTAC", hi)
    pairs = [primer.Pair("x", "AAGTAC", "GGTACC"), primer.Pair("y", "GGTACC", "AAGTRC")]
    assert thermo.panel_denoms(pairs, None) is None
    assert thermo.panel_denoms(pairs, d) == [a, thermo.denom_for_primer("GGTACC", d), thermo.denom_for_primer("GGTACC", d), 200.0]


# ---------------------------------------------------------------- formats and order

def test_go_g_format():
    for x, s in ((-0.0, "-0"), (0.0, "0"), (-18.975, "-18.975"), (-29.625, "-29.625"), (1e21, "1e+21"), (1e20, "1e+20"),
                 (1e6, "1e+06"), (123456789.0, "1.23456789e+08"), (999999.0, "999999"), (100000.0, "100000"), (0.0001, "0.0001"),
                 (0.00001234, "1.234e-05"), (0.1 + 0.2, "0.30000000000000004"), (12.65 * 1.5, "18.975"), (-100.0, "-100"),
                 (5e-324, "5e-324"), (1.7976931348623157e308, "1.7976931348623157e+308"), (2.5, "2.5"),
                 (float("nan"), "NaN"), (float("inf"), "+Inf"), (float("-inf"), "-Inf")):
        assert thermo.go_g(x) == s, (x, thermo.go_g(x))
    rng = random.Random(3)
    for _ in range(2000):                                               # shortest digits: the text reads back as the value
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if math.isnan(x) or math.isinf(x):
            continue
        assert float(thermo.go_g(x)) == x and float(thermo.go_json_float(x)) == x
    for x, s in ((-18.975, "-18.975"), (1e20, "100000000000000000000"), (1e21, "1e+21"), (1.5e-7, "1.5e-7"), (0.000001, "0.000001")):
        assert thermo.go_json_float(x) == s


def _prod(score, start, exp="e"):
    return engine.Product(exp, "s", start, start + 10, 10, "forward", 0, 0, (), (), Score=score)


def test_score_order_with_nan():
    ps = [_prod(-3.0, 5), _prod(float("nan"), 1), _prod(-0.0, 9), _prod(0.0, 2), _prod(-3.0, 4), _prod(float("nan"), 0),
          _prod(-29.625, 3), _prod(-18.975, 7)]
    rows = [("f", p, "") for p in ps]
    got = [(p.Score, p.Start) for _, p, _ in thermo_cli.sort_rows(rows, True)]
    assert [s for _, s in got] == [2, 9, 4, 5, 7, 3, 0, 1]                # higher first, ties and NaNs by coordinate, NaN last
    assert [p.Start for _, p, _ in thermo_cli.sort_rows(rows, False)] == [0, 1, 2, 3, 4, 5, 7, 9]
    assert thermo.score_rank(-0.0) == thermo.score_rank(0.0)           # a.Score != b.Score is false for the two zeros
    assert thermo.score_rank(1.0) < thermo.score_rank(-1.0) < thermo.score_rank(float("nan"))


def test_rows_and_jsonl():
    p = engine.Product("manual", "s", 0, 18, 18, "forward", 1, 0, (1,), (), Score=-18.975)
    assert thermo_cli.format_jsonl("a.fa", p, "ACGT") == ('{"experiment_id":"manual","sequence_id":"s","start":0,"end":18,"length":18,'
                                                         '"type":"forward","fwd_mm":1,"fwd_mm_i":[1],"seq":"ACGT","source_file":"a.fa",'
                                                         '"score":-18.975}')
    for z in (0.0, -0.0):                                               # omitempty: a zero of either sign is left out
        p.Score = z
        assert "score" not in thermo_cli.format_jsonl("a.fa", p, "ACGT")


# ---------------------------------------------------------------- the panel

def test_oligo_and_pair_construction(tmp_path):
    for c in LIT["oligo_inline"]:
        o = thermo_cli.parse_oligo_inline(c["spec"], c["index"])
        assert (o.ID, o.Seq) == (c["id"], c["seq"])
    for spec in LIT["oligo_inline_rejected"]:
        with pytest.raises(thermo_cli.UsageError):
            thermo_cli.parse_oligo_inline(spec, 0)
    assert thermo_cli.parse_oligo_inline("acgt", 2).ID == "O3"
    for c in LIT["oligo_tsv"]:
        path = tmp_path / "oligos.tsv"
        path.write_text(c["text"])
        assert [[o.ID, o.Seq] for o in thermo_cli.load_oligos_tsv(str(path))] == c["oligos"]
    for text in LIT["oligo_tsv_rejected"]:
        path = tmp_path / "bad.tsv"
        path.write_text(text)
        with pytest.raises(thermo_cli.UsageError):
            thermo_cli.load_oligos_tsv(str(path))
    ol = [primer.Oligo("A", "ACGT"), primer.Oligo("B", "GGCC"), primer.Oligo("C", "TTAA")]
    ps = thermo_cli.pairs_from_oligos(ol, 10, 500, True)
    assert [p.ID for p in ps] == ["A+B", "A+C", "B+C", "A+self", "B+self", "C+self"]
    assert (ps[0].Forward, ps[0].Reverse, ps[0].MinProduct, ps[0].MaxProduct) == ("ACGT", "GGCC", 10, 500)
    assert (ps[3].Forward, ps[3].Reverse, ps[3].MinProduct, ps[3].MaxProduct) == ("ACGT", "ACGT", 0, 0)
    assert [p.ID for p in thermo_cli.pairs_from_oligos(ol, 0, 0, False)] == ["A+B", "A+C", "B+C"]
    # through the parser: oligo mode, pair mode with the unique self pairs, Go's --self=false
    base = ["--thermo-model", "legacy-heuristic", "x.fa"]
    _, pairs, _ = thermo_cli.parse(base + ["--oligo", "a:acgt", "--oligo", "GGCC"])
    assert [p.ID for p in pairs] == ["a+O2", "a+self", "O2+self"]
    _, pairs, _ = thermo_cli.parse(base + ["-f", "aagtac", "-r", "GGTACC"])
    assert [(p.ID, p.Forward) for p in pairs] == [("manual", "AAGTAC"), ("manual+A:self", "AAGTAC"), ("manual+B:self", "GGTACC")]
    _, pairs, _ = thermo_cli.parse(base + ["-f", "AAGTAC", "-r", "GGTACC", "--self=false"])
    assert [p.ID for p in pairs] == ["manual"]
    o, _, salt = thermo_cli.parse(base + ["-f", "AAGTAC", "-r", "GGTACC", "--allow-indel", "--salt-model", "Owczarzy08"])
    assert o.allow_indel and salt == "owczarzy08" and (o.denom, o.rank, o.na, o.mg, o.dntp, o.primer_conc) == \
        ("fixed", "score", "50mM", "3mM", "0mM", "250nM")
    err = io.StringIO()
    c = thermo_cli.conditions(thermo_cli.parse(base + ["-f", "AAGTAC", "-r", "GGTACC", "--na", "lots"])[0], "monovalent", err)
    assert c.NaM == 0.05 and c.PrimerTotalM == 250 * 1e-9 and "bad --na" in err.getvalue() and "50mM" in err.getvalue()


# ---------------------------------------------------------------- what is not built is refused by name

REFUSED = [
    ([], "--thermo-model"),                                             # the reference's default is nn-structure-v1
    (["--thermo-model", "nn-duplex-v1"], "nn-duplex-v1"),
    (["--thermo-model", "nn-structure-v1"], "nn-structure-v1"),
    (["--thermo-model", "NN-Structure-V1"], "nn-structure-v1"),
    (["--thermo-model", "legacy-heuristic", "--single-stranded"], "--single-stranded"),
    (["--thermo-model", "legacy-heuristic", "--probe", "ACGTAC"], "--probe"),
    (["--thermo-model", "legacy-heuristic", "--thermo-details"], "--thermo-details"),
    (["--thermo-model", "legacy-heuristic", "--pretty"], "--pretty"),
    (["--thermo-model", "legacy-heuristic", "--output", "json"], "--output json"),
]


@pytest.mark.parametrize("extra,named", REFUSED)
def test_refusals_exit_2_without_a_device(extra, named, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refused run must not reach the engine")
    monkeypatch.setattr(thermo_cli.pipeline, "new_engine", no_device)
    out, err = io.StringIO(), io.StringIO()
    rc = thermo_cli.run(["-f", "AAGTAC", "-r", "GGTACC", "no_such_file.fa"] + extra, out, err)
    assert rc == 2 and out.getvalue() == ""
    assert named in err.getvalue() and "legacy-heuristic" in err.getvalue()


@pytest.mark.parametrize("extra", [["--thermo-model", "best"], ["--rank", "size"], ["--denom", "200"], ["--salt-model", "hidden-env"],
                                   ["--oligo", "a:ACGT"], ["--output", "xml"], ["--forward", ""]])
def test_usage_errors_exit_2(extra, monkeypatch):
    monkeypatch.setattr(thermo_cli.pipeline, "new_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("engine")))
    argv = ["-f", "AAGTAC", "-r", "GGTACC", "x.fa", "--thermo-model", "legacy-heuristic"]
    if extra == ["--forward", ""]:
        argv = ["-r", "GGTACC", "x.fa", "--thermo-model", "legacy-heuristic"]
    err = io.StringIO()
    assert thermo_cli.run(argv + extra, io.StringIO(), err) == 2 and err.getvalue()


def test_abi_declares_the_thermo_entry_points():
    hdr = open(os.path.join(os.path.dirname(R.GOLDEN), "..", "..", "include", "ipcr_hip.h")).read()
    assert "#define IPCR_ABI_VERSION 6" in hdr
    for name in ("ipcr_thermo_legacy_products", "ipcr_thermo_legacy_scratch_products", "ipcr_thermo_legacy_penalty",
                 "ipcr_thermo_mismatch_ddg"):
        assert name in hdr and name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
