"""--products and --output fasta of the CLI, without a GPU: the JSONL `seq` field and the FASTA records of
internal/output/fasta.go against literal lines, with both index rules of internal/writers/product.go:66-80."""
import io

from ipcr_amd import cli, engine


def prod(exp, start, end, fmm=0, rmm=0, fi=(), ri=()):
    return engine.Product(ExperimentID=exp, SequenceID="chr1", Start=start, End=end, Length=end - start, Type="forward",
                          FwdMM=fmm, RevMM=rmm, FwdMismatchIdx=tuple(fi), RevMismatchIdx=tuple(ri))


def test_jsonl_seq_field_order():
    p = prod("C3", 10, 30, 1, 2, (3,), (0, 4))
    assert cli.format_jsonl("g.fa", p) == (
        '{"experiment_id":"C3","sequence_id":"chr1","start":10,"end":30,"length":20,"type":"forward","fwd_mm":1,'
        '"rev_mm":2,"fwd_mm_i":[3],"rev_mm_i":[0,4],"source_file":"g.fa"}')
    assert cli.format_jsonl("g.fa", p, "ACGRY-N") == (
        '{"experiment_id":"C3","sequence_id":"chr1","start":10,"end":30,"length":20,"type":"forward","fwd_mm":1,'
        '"rev_mm":2,"fwd_mm_i":[3],"rev_mm_i":[0,4],"seq":"ACGRY-N","source_file":"g.fa"}')
    assert cli.format_jsonl("", prod("a", 0, 4), "AC<T") == (
        '{"experiment_id":"a","sequence_id":"chr1","start":0,"end":4,"length":4,"type":"forward","seq":"AC\\u003cT"}')
    assert cli.format_jsonl("g.fa", p, "") == cli.format_jsonl("g.fa", p)


def test_fasta_records_and_index_rules():
    rows = [("g.fa", prod("p1", 5, 9), "ACGT"), ("g.fa", prod("p1", 7, 7), ""), ("h.fa", prod("p2", 100, 104), "RYN-")]
    # StreamFASTA: the index counts the records written (the empty product is skipped and not counted)
    assert cli.fasta_records(rows, sort=False) == [
        ">p1_1 start=5 end=9 len=4 source_file=g.fa\nACGT",
        ">p2_2 start=100 end=104 len=4 source_file=h.fa\nRYN-",
    ]
    # WriteFASTA (--sort): the index is the position in the sorted list + 1
    assert cli.fasta_records(rows, sort=True) == [
        ">p1_1 start=5 end=9 len=4 source_file=g.fa\nACGT",
        ">p2_3 start=100 end=104 len=4 source_file=h.fa\nRYN-",
    ]
    assert cli.format_fasta(7, "x.fa", prod("C3", 1, 3), "AC") == ">C3_7 start=1 end=3 len=2 source_file=x.fa\nAC"


def test_parser_takes_the_new_options():
    o = cli.build_parser().parse_args(["-f", "ACGT", "-r", "ACGT", "--products", "-o", "fasta", "x.fa"])
    assert o.products and o.output == "fasta"


def test_probe_with_sequences_is_refused(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">s\nACGTACGTACGT\n")
    for extra in (["--output", "fasta"], ["--products"]):
        out, err = io.StringIO(), io.StringIO()
        rc = cli.run(["-f", "ACGTACGTAC", "-r", "ACGTACGTAC", "--probe", "ACGTAC", *extra, str(fa)], stdout=out, stderr=err)
        assert rc == 2, extra
        assert "--probe" in err.getvalue()


def test_both_drivers_take_the_common_flags_with_the_same_defaults():
    """internal/clibase/common.go:61-110: one set of common flags under ipcr, ipcr-probe, ipcr-multiplex and ipcr-nested"""
    from ipcr_amd import nested_cli
    common = [  # (flag, short form, destination, default, a value to parse, what it parses to)
        ("--sequences", "-s", "sequences", [], "a.fa", ["a.fa"]),
        ("--mismatches", "-m", "mismatches", 0, "2", 2),
        ("--min-length", None, "min_length", 0, "5", 5),
        ("--max-length", None, "max_length", 2000, "50", 50),
        ("--hit-cap", None, "hit_cap", 10000, "7", 7),
        ("--terminal-window", None, "terminal_window", 3, "-1", -1),
        ("--no-self", None, "self_", True, None, False),
        ("--self", None, "self_", True, None, True),
        ("--seed-length", None, "seed_length", 12, "8", 8),
        ("--circular", "-c", "circular", False, None, True),
        ("--sort", None, "sort", False, None, True),
        ("--output", "-o", "output", "text", "jsonl", "jsonl"),
        ("--no-header", None, "no_header", False, None, True),
        ("--no-match-exit-code", None, "no_match_exit_code", 0, "7", 7),
        ("--chunk-size", None, "chunk_size", 0, "4000", 4000),
        ("--dedup-cap", None, "dedup_cap", 0, "9", 9),
        ("--device", None, "device", 0, "1", 1),
    ]
    for build in (cli.build_parser, nested_cli.build_parser):
        defaults = vars(build().parse_args([]))
        assert defaults["fasta"] == []
        for flag, short, dest, default, text, value in common:
            assert defaults[dest] == default, (build.__module__, flag)
            for name in filter(None, (flag, short)):
                o = build().parse_args([name] + ([text] if text is not None else []) + ["x.fa", "y.fa"])
                assert getattr(o, dest) == value and o.fasta == ["x.fa", "y.fa"], (build.__module__, name)
