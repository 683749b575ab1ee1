"""CPU checks of tests/launch_trace.py and tests/dispatch_tables.py: the parser of demangled kernel names on literal strings, and that
every kernel of the k-NN and GEMM sources has a row in the dispatch tables (a kernel added later without one fails here)."""
import glob
import os
import re

import pytest

from launch_trace import parse_kernel_name, find, assert_launched
import dispatch_tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-gcnn_amd", "csrc")

NAMES = [
    ("void (anonymous namespace)::knn_mfma_kernel<64, 20, true>(float const*, float const*, int, int, long, int, int*, float const*)",
     ("knn_mfma_kernel", ["64", "20", "true"])),
    ("void (anonymous namespace)::knn_kernel<4, 20, (anonymous namespace)::PackedClouds>(float const*, float const*, "
     "(anonymous namespace)::PackedClouds, int, long, int, int, int*, float const*)", ("knn_kernel", ["4", "20", "PackedClouds"])),
    ("void (anonymous namespace)::gemm_kernel<0, 1, 0, 128, 64, false>((anonymous namespace)::GemmP)",
     ("gemm_kernel", ["0", "1", "0", "128", "64", "false"])),
    # a plain kernel: no return type in the demangled form of a non-template function
    ("(anonymous namespace)::sqnorm_kernel(float const*, long, long, int, float*)", ("sqnorm_kernel", [])),
    ("sqnorm_kernel", ("sqnorm_kernel", [])),
    ("void dg::detail::colsum_kernel(float const*, int)", ("colsum_kernel", [])),
    # nested template types stay one argument; their namespaces go
    ("void k<std::tuple<int, ns::Pair<float, 3> >, 7>(std::tuple<int, ns::Pair<float, 3> >)", ("k", ["tuple<int, Pair<float, 3>>", "7"])),
    ("void (anonymous namespace)::scan<(anonymous namespace)::Cfg<16, (anonymous namespace)::DenseClouds>, 2>(int)",
     ("scan", ["Cfg<16, DenseClouds>", "2"])),
    # bool and negative integer arguments, with and without the cast older demanglers print
    ("void f<(bool)1, (bool)0, (int)-3>(float*)", ("f", ["true", "false", "-3"])),
    ("void f<true, false, -3, 4u>(float*)", ("f", ["true", "false", "-3", "4u"])),
    ("void (anonymous namespace)::knn_grid_query_kernel<20, false, true, (anonymous namespace)::DenseClouds>(HIP_vector_type<float, 4u> "
     "const*, float const*, int const*, int const*, (anonymous namespace)::GridInfo const*, (anonymous namespace)::DenseClouds, int, int*)",
     ("knn_grid_query_kernel", ["20", "false", "true", "DenseClouds"])),
    # a function-pointer parameter does not end the parameter list early
    ("void ns::apply<8>(void (*)(int, float), int)", ("apply", ["8"])),
    ("unsigned int ns::count<2>(int)", ("count", ["2"])),
]

RAW = ["_ZN12_GLOBAL__N_115knn_mfma_kernelILi64ELi20ELb1EEEvPKfS2_iiliPiS2_", "_Z3fooIXadL_Z3barEEEvv.kd", ""]


@pytest.mark.parametrize("s,want", NAMES, ids=[w[0] + str(i) for i, (_, w) in enumerate(NAMES)])
def test_parse_kernel_name(s, want):
    assert parse_kernel_name(s) == want


@pytest.mark.parametrize("s", RAW)
def test_a_string_that_does_not_demangle_comes_back_whole(s):
    assert parse_kernel_name(s) == (s, [])


def test_find_matches_leading_arguments_and_wildcards():
    L = [("sqnorm_kernel", [], (5, 1, 1), (256, 1, 1), 0), ("knn_mfma_kernel", ["64", "20", "true"], (5, 2, 1), (256, 1, 1), 0)]
    assert find(L, "knn_mfma_kernel") and find(L, "knn_mfma_kernel", [64, 20]) and find(L, "knn_mfma_kernel", ["*", "20", "true"])
    assert not find(L, "knn_mfma_kernel", [16]) and not find(L, "knn_kernel") and not find(L, "sqnorm_kernel", ["1"])
    assert_launched(L, "sqnorm_kernel")
    with pytest.raises(AssertionError):
        assert_launched(L, "knn_mfma_kernel", [64, 20, "false"])


# ------------------------------------------------------------------------------------------------------
def kernels_of_the_sources():
    files = sorted(glob.glob(os.path.join(CSRC, "knn*.hip"))) + [os.path.join(CSRC, f) for f in ("knn_scan.h", "gemm.hip", "gemm_x3.hip")]
    out = {}
    for f in files:
        text = open(f).read()
        for m in re.finditer(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", text, flags=re.S):
            out[m.group(1)] = os.path.basename(f)
    return out


def rows_of_the_tables():
    return T.KNN_DENSE + T.KNN_PACKED + T.KNN_CROSS + T.GEMM


def test_every_kernel_of_the_knn_and_gemm_sources_has_a_row():
    found = kernels_of_the_sources()
    assert len(found) >= 20 and "knn_bf16a_kernel" in found and "gemm_x3q_kernel" in found, found
    expected = {e[0] for r in rows_of_the_tables() for e in r["expect"]}
    assert expected <= set(found), "rows name kernels the sources do not have: %s" % sorted(expected - set(found))
    assert not (set(T.NOT_DISPATCHED) & expected), "a kernel is both in a row and in NOT_DISPATCHED"
    assert set(T.NOT_DISPATCHED) <= set(found), sorted(set(T.NOT_DISPATCHED) - set(found))
    missing = sorted(set(found) - expected - set(T.NOT_DISPATCHED))
    assert not missing, "kernels without a row in tests/dispatch_tables.py: %s" % [(k, found[k]) for k in missing]


def test_row_ids_are_unique_and_rows_are_literal():
    for table in (T.KNN_DENSE, T.KNN_PACKED, T.KNN_CROSS, T.GEMM):
        ids = [r["id"] for r in table]
        assert len(ids) == len(set(ids))
        for r in table:
            assert r["expect"] and all(isinstance(n, str) and all(isinstance(a, str) for a in a_) for n, a_ in r["expect"]), r["id"]


# ------------------------------------------------------------------------------------------------------
def test_the_24_bit_multiply_has_one_caller():
    """HIP declares __umul24 as returning int; a gathered row's offset may be 2^31 elements or more and must enter its address
    zero-extended.  common.h:row_offset24 is the one place that calls it (and returns unsigned) and whose comment carries the
    contract: nowhere else in csrc does the name occur, in code or in a comment that would invite a copy."""
    name = "__umul24"
    hits = []
    for f in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(f):
            for n, line in enumerate(open(f, errors="replace").read().split("\n"), 1):
                if name in line:
                    hits.append((os.path.basename(f), n, line))
    assert hits and {h[0] for h in hits} == {"common.h"}, [h[:2] for h in hits]
    lines = open(os.path.join(CSRC, "common.h")).read().split("\n")
    code = [h for h in hits if name in h[2].split("//")[0]]
    assert len(code) == 1 and re.search(r"\bunsigned\s+row_offset24\s*\(\s*unsigned\s+\w+\s*,\s*unsigned\s+\w+\s*\)", code[0][2]), code
    # the other occurrences: the comment block that ends at the definition
    assert max(h[1] for h in hits) == code[0][1]
    first = min(h[1] for h in hits)
    block = lines[first - 1:code[0][1] - 1]
    assert all(l.startswith("//") for l in block), "the name occurs outside row_offset24 and its comment"
    assert any("row_offset24(" in open(os.path.join(CSRC, f)).read() for f in ("bn.hip", "seg_bn.hip", "misc.hip"))
