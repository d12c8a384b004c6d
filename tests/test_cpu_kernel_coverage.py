"""tools/kernel_coverage.py: name normalisation, trace reading and the --expect gate (no compiler, no GPU: the compiled list is handed in)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_names_are_normalised_the_same_way_from_symbols_and_from_traces():
    K = _tool()
    want = "gspn_k::fwd_short_kernel<16, 2, 1, true, false>"
    assert K.strip_args("void gspn_k::fwd_short_kernel<16, 2, 1, true, false>(int, int, int, float const*, gspn_k::PoolOut) [clone .kd]") == want
    assert K.strip_args("void gspn_k::fwd_short_kernel<16, 2, 1, true, false>(int, int, int, float const*, gspn_k::PoolOut)") == want
    assert K.strip_args("bn_finalize_kernel(long, int, float const*)") == "bn_finalize_kernel"
    assert K.strip_args("pool_select_kernel(long, int, PoolOut, float const*).kd") == "pool_select_kernel"
    assert K.strip_args("void (anonymous namespace)::k<(anonymous namespace)::T, 4>((anonymous namespace)::T*)") == "(anonymous namespace)::k<(anonymous namespace)::T, 4>"
    assert K.strip_args("Cijk_Ailk_Bljk_SB_MT64x32x16") == "Cijk_Ailk_Bljk_SB_MT64x32x16"
    assert K.template_of(want) == "gspn_k::fwd_short_kernel" and K.template_of("bn_finalize_kernel") == "bn_finalize_kernel"
    assert K.template_of("(anonymous namespace)::box_point_count_kernel<4>") == "(anonymous namespace)::box_point_count_kernel"
    # a mangled symbol and its demangled trace name meet
    assert K.normalise(["_Z18bn_finalize_kernelliPKf", "bn_finalize_kernel(long, int, float const*)"]) == ["bn_finalize_kernel"]


def test_executed_reads_every_process_s_trace_and_expect_gates(tmp_path, monkeypatch, capsys):
    K = _tool()
    comp = ["k<1, false>", "k<1, true>", "k<2, false>", "plain_kernel"]
    monkeypatch.setattr(K, "compiled", lambda sources=(): list(comp))
    d = tmp_path / "trace" / "host"
    d.mkdir(parents=True)
    (d / "100_kernel_trace.csv").write_text('"Kind","Kernel_Name","Start_Timestamp"\n"KERNEL_DISPATCH","void k<1, false>(int, float*)",1\n'
                                            '"KERNEL_DISPATCH","plain_kernel(long)",2\n')
    (d / "101_kernel_trace.csv").write_text('"Kind","Kernel_Name","Start_Timestamp"\n"KERNEL_DISPATCH","void k<2, false>(int, float*) [clone .kd]",1\n')   # a child process
    (d / "100_agent_info.csv").write_text('"Node_Id","Name"\n0,"gfx950"\n')
    rec = tmp_path / "record.txt"
    rec.write_text("# comment\n[compiled]\nk<1, false>\nk<1, true>\n\n[executed after]\nk<1, false>   # note\nk<2, false>\n\n[not executed]\nk<1, true>    # a switch\n")
    assert K.read_section(str(rec), "executed after") == ["k<1, false>", "k<2, false>"]
    assert K.main(["executed", str(tmp_path / "trace"), "--expect", str(rec)]) == 0
    out = capsys.readouterr().out
    assert "not executed (1):" in out and "  k<1, true>" in out
    rec.write_text("[executed after]\nk<1, false>\nk<1, true>\n")
    assert K.main(["executed", str(tmp_path / "trace"), "--expect", str(rec)]) == 1
    assert "k<1, true>" in capsys.readouterr().out.split("in no trace")[1]


def test_the_two_records_partition_the_compiled_list():
    """profiles/kernel_coverage_geometry.txt covers exactly what profiles/kernel_coverage_mlp.txt compiles and does not account for; every
    instantiation is in one of [executed after] and [not executed], what ran before still runs, and each [not executed] line has its reason"""
    K = _tool()
    mlp = os.path.join(ROOT, "profiles", "kernel_coverage_mlp.txt")
    geo = os.path.join(ROOT, "profiles", "kernel_coverage_geometry.txt")
    compiled = K.read_section(mlp, "compiled")
    theirs = K.read_section(mlp, "executed after") + K.read_section(mlp, "not executed")
    before, after, never = (K.read_section(geo, s) for s in ("executed before", "executed after", "not executed"))
    assert len(set(after + never)) == len(after) + len(never)
    assert sorted(theirs + after + never) == sorted(compiled)
    assert set(before) <= set(after)
    for want in ["crop_linear_fwd_kernel<%d>" % l for l in (2, 4, 8, 64)] + ["crop_linear_bwd_side_kernel<%d>" % l for l in (2, 4, 8, 64)]:
        assert "(anonymous namespace)::" + want in after
    for want in ["three_nn_nested_kernel<%d>" % l for l in (1, 2, 4)] + ["three_nn_grid_kernel<32>", "nm_distance_kernel<2>"]:
        assert want in after
    assert "(anonymous namespace)::box_point_count_kernel<8>" in after
    with open(geo) as fh:
        body = fh.read().split("\n[not executed]\n")[1]
    lines = [l for l in body.splitlines() if l.strip()]
    assert len(lines) == len(never) and all(len(l.split("#", 1)[1].strip()) > 20 for l in lines)
