"""The `ipcr-nested` driver without a GPU: TSV header and rows (internal/nestedoutput/text.go), api.NestedProductV1 as
encoding/json writes it (pkg/api/nested_v1.go: field order, omitempty), the usage errors of nestedcli.ParseArgs /
clibase.Validate (exit 2), the writer registry's refusal of fasta (exit 3) and the stable LessProduct sort."""
import io
import json

import pytest

from ipcr_amd import engine, nested, nested_cli


def prod(exp="outer", seq_id="chr1", start=10, end=30, fmm=0, rmm=0, fi=(), ri=(), typ="forward"):
    return engine.Product(ExperimentID=exp, SequenceID=seq_id, Start=start, End=end, Length=end - start, Type=typ,
                          FwdMM=fmm, RevMM=rmm, FwdMismatchIdx=tuple(fi), RevMismatchIdx=tuple(ri))


def found(p, start=0, end=8, fmm=0, rmm=0, pair="inner", typ="forward"):
    return nested.NestedProduct(p, True, pair, start, end, end - start, typ, fmm, rmm)


def test_header_and_rows():
    assert nested_cli.TSV_HEADER_NESTED == (
        "source_file\tsequence_id\touter_experiment_id\touter_start\touter_end\touter_length\touter_type\t"
        "inner_experiment_id\tinner_found\tinner_start\tinner_end\tinner_length\tinner_type\tinner_fwd_mm\tinner_rev_mm")
    assert len(nested_cli.TSV_HEADER_NESTED.split("\t")) == 15
    # nestedoutput/text_test.go: a found inner product at 0 prints its zeros
    np = found(prod(seq_id="s:0-8", start=0, end=8), 0, 4)
    assert nested_cli.format_row("ref.fa", np) == "ref.fa\ts:0-8\touter\t0\t8\t8\tforward\tinner\ttrue\t0\t4\t4\tforward\t0\t0"
    np = found(prod(start=5, end=305, fmm=1, typ="revcomp"), 17, 117, fmm=1, rmm=2, pair="in2", typ="revcomp")
    assert nested_cli.format_row("g.fa", np) == "g.fa\tchr1\touter\t5\t305\t300\trevcomp\tin2\ttrue\t17\t117\t100\trevcomp\t1\t2"
    # no inner product: every inner field empty, the pair ID too
    np = nested.NestedProduct(prod(), False)
    assert nested_cli.format_row("g.fa", np) == "g.fa\tchr1\touter\t10\t30\t20\tforward\t\tfalse\t\t\t\t\t\t"
    assert len(nested_cli.format_row("g.fa", np).split("\t")) == 15


def test_jsonl_field_order_and_omitempty():
    p = prod(fmm=1, rmm=2, fi=(3,), ri=(0, 4))
    # inner_start 0 is left out even though the inner product was found; zero mismatches too
    assert nested_cli.format_jsonl("g.fa", found(p, 0, 8), "ACGTNNRY") == (
        '{"experiment_id":"outer","sequence_id":"chr1","start":10,"end":30,"length":20,"type":"forward","fwd_mm":1,'
        '"rev_mm":2,"fwd_mm_i":[3],"rev_mm_i":[0,4],"seq":"ACGTNNRY","source_file":"g.fa","inner_found":true,'
        '"inner_experiment_id":"inner","inner_end":8,"inner_length":8,"inner_type":"forward"}')
    assert nested_cli.format_jsonl("g.fa", found(p, 2, 9, fmm=1, rmm=1), "AC") == (
        '{"experiment_id":"outer","sequence_id":"chr1","start":10,"end":30,"length":20,"type":"forward","fwd_mm":1,'
        '"rev_mm":2,"fwd_mm_i":[3],"rev_mm_i":[0,4],"seq":"AC","source_file":"g.fa","inner_found":true,'
        '"inner_experiment_id":"inner","inner_start":2,"inner_end":9,"inner_length":7,"inner_type":"forward",'
        '"inner_fwd_mm":1,"inner_rev_mm":1}')
    # inner_found is never omitted; outer start 0 is not omitempty; <, >, & escaped as encoding/json does
    assert nested_cli.format_jsonl("", nested.NestedProduct(prod(start=0, end=4), False), "A<&>") == (
        '{"experiment_id":"outer","sequence_id":"chr1","start":0,"end":4,"length":4,"type":"forward",'
        '"seq":"A\\u003c\\u0026\\u003e","inner_found":false}')


def test_json_array_is_indented_like_encode_pretty():
    rows = [("g.fa", found(prod(fi=(1, 2)), 3, 9), "ACGT"), ("g.fa", nested.NestedProduct(prod(start=40, end=60), False), "GG")]
    assert nested_cli.format_json(rows) == """[
  {
    "experiment_id": "outer",
    "sequence_id": "chr1",
    "start": 10,
    "end": 30,
    "length": 20,
    "type": "forward",
    "fwd_mm_i": [
      1,
      2
    ],
    "seq": "ACGT",
    "source_file": "g.fa",
    "inner_found": true,
    "inner_experiment_id": "inner",
    "inner_start": 3,
    "inner_end": 9,
    "inner_length": 6,
    "inner_type": "forward"
  },
  {
    "experiment_id": "outer",
    "sequence_id": "chr1",
    "start": 40,
    "end": 60,
    "length": 20,
    "type": "forward",
    "seq": "GG",
    "source_file": "g.fa",
    "inner_found": false
  }
]
"""
    assert nested_cli.format_json([]) == "[]\n"
    assert [json.loads(nested_cli.format_jsonl(*r)) for r in rows] == json.loads(nested_cli.format_json(rows))


def test_sort_is_stable_less_product():
    a = ("g.fa", nested.NestedProduct(prod(start=50, end=70), False), "A")
    b = ("g.fa", found(prod(start=10, end=30)), "C")
    c = ("g.fa", nested.NestedProduct(prod(seq_id="chr1:0-100", start=5, end=25), False), "G")  # chunk suffix: base chr1, 5
    d = ("a.fa", nested.NestedProduct(prod(start=900, end=920), False), "T")
    e1 = ("g.fa", found(prod(start=10, end=30), 1, 5), "C")                         # ties with b on every key
    e2 = ("g.fa", found(prod(start=10, end=30), 2, 6), "C")
    got = nested_cli.sort_rows([a, b, e1, c, d, e2])
    assert got == [d, c, b, e1, e2, a]
    assert nested_cli.sort_rows([e2, b, e1]) == [e2, b, e1]
    # Seq is LessProduct's last key
    s1 = ("g.fa", nested.NestedProduct(prod(), False), "T")
    s2 = ("g.fa", nested.NestedProduct(prod(), False), "A")
    assert nested_cli.sort_rows([s1, s2]) == [s2, s1]


@pytest.mark.parametrize("args,msg", [
    (["-F", "ACGTACGT", "-R", "ACGTACGT", "g.fa"], "provide --primers or --forward/--reverse"),
    (["-f", "ACGTACGT", "-F", "ACGTACGT", "-R", "ACGTACGT", "g.fa"], "--forward and --reverse must be supplied together"),
    (["-p", "o.tsv", "-f", "ACGT", "-r", "ACGT", "-F", "ACGT", "-R", "ACGT", "g.fa"], "--primers conflicts with"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "g.fa"], "provide --inner-primers or --inner-forward/--inner-reverse"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "g.fa"], "--inner-forward and --inner-reverse must be supplied together"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-R", "ACGT", "g.fa"], "--inner-forward and --inner-reverse must be supplied together"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-P", "i.tsv", "-F", "ACGT", "-R", "ACGT", "g.fa"],
     "--inner-primers conflicts with --inner-forward/--inner-reverse"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGTX", "-R", "ACGT", "g.fa"], "--inner-forward: invalid primer base"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "AC!", "g.fa"], "--inner-reverse: invalid primer base"),
    (["-f", "ACGTACJT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "g.fa"], "--forward: invalid primer base"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT"], "at least one sequence file is required"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "-o", "pretty", "g.fa"], 'invalid --output "pretty"'),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "--chunk-size", "-1", "g.fa"], "--chunk-size"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "--terminal-window", "-2", "g.fa"], "--terminal-window"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "--no-match-exit-code", "256", "g.fa"], "--no-match-exit-code"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "--max-length", "5", "g.fa"],
     "effective maximum product length (5) is smaller than the longest primer length (8)"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "--min-length", "300", "--max-length", "200", "g.fa"],
     "--min-length (300) exceeds --max-length (200)"),
    (["-f", "ACGTACGT", "-r", "ACGTACGT", "-P", "/nonexistent/inner.tsv", "g.fa"], "inner.tsv"),
])
def test_usage_errors_exit_2(args, msg):
    out, err = io.StringIO(), io.StringIO()
    assert nested_cli.run(args, stdout=out, stderr=err) == 2
    assert msg in err.getvalue()
    assert out.getvalue() == ""


def test_malformed_flag_exits_2(capsys):
    assert nested_cli.run(["--mismatches", "x", "-f", "ACGT", "-r", "ACGT", "g.fa"]) == 2


def test_fasta_output_is_refused_like_write_nested():
    out, err = io.StringIO(), io.StringIO()
    rc = nested_cli.run(["-f", "ACGTACGT", "-r", "ACGTACGT", "-F", "ACGT", "-R", "ACGT", "-o", "fasta", "g.fa"], stdout=out, stderr=err)
    assert rc == 3
    assert 'unknown nested format "fasta" (no writer registered)' in err.getvalue()


def test_pairs_ids_bounds_and_self(tmp_path):
    _, outer, inner = nested_cli.parse(["-f", "acgtac gtac", "-r", "TTGGCCAA", "-F", "gattaca", "-R", "CCGG",
                                        "--min-length", "50", "--max-length", "900", "g.fa"])
    assert [(p.ID, p.Forward, p.Reverse, p.MinProduct, p.MaxProduct) for p in outer] == [
        ("outer", "ACGTACGTAC", "TTGGCCAA", 50, 900), ("outer+A:self", "ACGTACGTAC", "ACGTACGTAC", 0, 0),
        ("outer+B:self", "TTGGCCAA", "TTGGCCAA", 0, 0)]
    assert [(p.ID, p.Forward, p.Reverse, p.MinProduct, p.MaxProduct) for p in inner] == [
        ("inner", "GATTACA", "CCGG", 0, 0), ("inner+A:self", "GATTACA", "GATTACA", 0, 0), ("inner+B:self", "CCGG", "CCGG", 0, 0)]
    ti = tmp_path / "i.tsv"
    ti.write_text("# inner\nin1 ACGTACGT TTGGCCAA 10 200\nin2 GGGGCCCC AAAATTTT\n")
    o, outer, inner = nested_cli.parse(["--outer-primers", str(ti), "--inner-primers", str(ti), "--no-self", "g.fa"])
    assert [p.ID for p in outer] == ["in1", "in2"] and [p.ID for p in inner] == ["in1", "in2"]
    assert (inner[0].MinProduct, inner[0].MaxProduct) == (10, 200)
    assert nested_cli.effective_max_len(2000, outer) == 2000
    assert nested_cli.effective_max_len(100, outer) == 200
    assert nested_cli.effective_max_len(0, outer) == 0
