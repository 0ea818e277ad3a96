"""tools/kernel_coverage.py on a hand-written symbol list and hand-written traces (tests/golden/kernel_coverage): the
three sets of `diff`, with names that differ only in template arguments and in whitespace."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "kernel_coverage")


@pytest.fixture(scope="module")
def kc():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_normalize(kc):
    n = kc.normalize
    assert n("void k<64, 128 >(float const*, int) [clone .kd]") == "k<64,128>"
    assert n("void k<64,128>(float const*, int)") == "k<64,128>"
    assert n("k<64, 128>") == "k<64,128>"
    assert n("bev_sum_kernel(float const*, int)") == "bev_sum_kernel"
    assert n("bev_sum_kernel.kd") == "bev_sum_kernel"
    assert n("void mode_kernel<(Mode)1>(float*)") == "mode_kernel<(Mode)1>"
    assert n("void g<unsigned int, 2u>(HIP_vector_type<int, 2u> const*)") == "g<unsigned int,2u>"
    assert n("_Z15pack_dma_kernelPKDF16_iiiPDF16_l") == "pack_dma_kernel"
    assert n("void k<0, 2>(P)") != n("void k<0, 1>(P)") != n("void k<1, 2>(P)")


def test_diff_three_sets(kc):
    lib = kc.read_symbols(os.path.join(G, "symbols.txt"))
    assert len(lib) == 12
    d = kc.diff(lib, [os.path.join(G, "trace_kernel_stats.csv")])
    assert d["launched"] == ["bev_sum_kernel", "conv3x3_f16x3_frag_kernel<0,1>", "conv3x3_f16x3_frag_kernel<0,2>",
                             "greedy_kernel<double>", "mode_kernel<(Mode)1>", "pack_dma_kernel",
                             "sp_conv_r16_kernel<16,4,2,48,true>", "sp_conv_wave2_kernel<128,128,8,2,2,2>"]
    assert d["never"] == ["bev_sum_vec_kernel", "conv3x3_f16x3_frag_kernel<1,2>", "sp_conv_r16_kernel<16,4,2,48,false>",
                          "sp_conv_wave2_kernel<128,128,16,2,2,2>"]
    assert d["foreign"] == ["Cijk_Ailk_Bljk_SB_MT64x64x16_SN_K1", "at::native::vectorized_elementwise_kernel<4,"
                            "at::native::FillFunctor<float>,std::array<char*,1ul>>"]
    assert list(d["rows"].values()) == [10]
    assert set(d["launched"]) | set(d["never"]) == set(lib) and not set(d["launched"]) & set(d["never"])


def test_diff_merges_traces(kc):
    lib = kc.read_symbols(os.path.join(G, "symbols.txt"))
    d = kc.diff(lib, [os.path.join(G, "trace_kernel_stats.csv"), os.path.join(G, "trace_child.txt")])
    assert "sp_conv_wave2_kernel<128,128,16,2,2,2>" in d["launched"]
    assert d["never"] == ["bev_sum_vec_kernel", "conv3x3_f16x3_frag_kernel<1,2>", "sp_conv_r16_kernel<16,4,2,48,false>"]
    assert list(d["rows"].values()) == [10, 1]
    # a directory is searched for *kernel_stats.csv
    assert kc.diff(lib, [G])["never"] == kc.diff(lib, [os.path.join(G, "trace_kernel_stats.csv")])["never"]


def test_cli_prints_the_sets(kc, capsys):
    assert kc.main(["diff", "--symbols", os.path.join(G, "symbols.txt"), os.path.join(G, "trace_kernel_stats.csv")]) == 0
    out = capsys.readouterr().out
    head, rest = out.split("[launched]\n")
    launched, rest = rest.split("[never launched]\n")
    never, foreign = rest.split("[launched, not in the library]\n")
    assert "launched 8, never launched 4, launched but not in the library 2" in head
    assert "conv3x3_f16x3_frag_kernel<1,2>" in never.split() and "conv3x3_f16x3_frag_kernel<0,2>" in launched.split()
    assert len(foreign.strip().splitlines()) == 2
