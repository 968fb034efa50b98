"""CPU-only: the scorer launchers' choice of kernel form (csrc/mgfn.hip) through the library's form queries -- the rule each
launcher itself calls.  Every case of tests/test_hip_scorer_forms.py is pinned to the form it is there to reach, and every threshold
to both of its sides: if a threshold moves, this fails instead of the GPU cases quietly running another kernel."""
import ctypes as C
import os
import re

import pytest

import scorer_form_cases as cases
from conftest import REPO

QUERIES = ("advhip_bn_rows_form", "advhip_chan_layernorm_form", "advhip_head_ln_fc_form", "advhip_dwconv_t_form")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    return _lib.load()


def test_queries_are_declared_bound_and_exported_and_the_abi_version_is_still_2(lib):
    from anomaly_detection_on_video_amd import _lib

    assert lib.advhip_abi_version() == 2
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    assert re.search(r"#define\s+ADVHIP_ABI_VERSION\s+2\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in QUERIES:
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/advhip.h"
        declared = (ctype[m.group(1)], [ctype[a.split()[0]] for a in m.group(2).split(",")])
        assert _lib.SIGNATURES[name] == declared, name
        assert hasattr(lib, name), f"{name} is not exported"
    for macro, value in (("GENERIC", cases.BN_GENERIC), ("REG256X4", cases.BN_REG256X4), ("REG256X12", cases.BN_REG256X12), ("REG1024X4", cases.BN_REG1024X4)):
        assert re.search(rf"#define\s+ADVHIP_BN_ROWS_{macro}\s+{value}\b", text), macro
    assert (_lib.BN_ROWS_GENERIC, _lib.BN_ROWS_REG256X4, _lib.BN_ROWS_REG256X12, _lib.BN_ROWS_REG1024X4) == (0, 1, 2, 3)


def _check(lib, what, table):
    for *shape, form in table:
        assert cases.query(lib, what, *shape, 1) == form, (what, shape, "aligned")
        assert cases.query(lib, what, *shape, 0) == 0, (what, shape, "an operand on a 4-byte boundary")


def test_every_gpu_case_takes_the_form_it_is_there_for(lib):
    _check(lib, "bn_rows", cases.BN_CASES)
    _check(lib, "chan_layernorm", cases.LN_CASES)
    _check(lib, "head_ln_fc", cases.HEAD_CASES)
    _check(lib, "dwconv_t", [(t, form) for _k, t, form in cases.DW_CASES])
    for name, table in (("bn_rows", cases.BN_CASES), ("chan_layernorm", cases.LN_CASES), ("head_ln_fc", cases.HEAD_CASES), ("dwconv_t", cases.DW_CASES)):
        reached = {(name, row[-1]) for row in table}
        assert reached == {f for f in cases.ALL_FORMS if f[0] == name}, name  # the tables reach every form of the query
    for c, h, rows, chunks in cases.DW_GEOMETRIES:
        assert lib.advhip_dwconv_t_bwd_chunks(c, rows) == chunks, (c, rows)
    for shape, table in ((cases.BN_BIG_MEAN, cases.BN_CASES), (cases.LN_BIG_MEAN, cases.LN_CASES), (cases.HEAD_BIG_MEAN, cases.HEAD_CASES),
                         (cases.HEAD_SATURATED, cases.HEAD_CASES), (cases.DW_BIG_MEAN, cases.DW_CASES)):
        assert [row[-1] for row in table if tuple(row[:-1]) == shape] not in ([], [0]), shape  # on a register / 16-byte form


def test_bn_rows_thresholds_from_both_sides(lib):
    g, r4, r12, w = cases.BN_GENERIC, cases.BN_REG256X4, cases.BN_REG256X12, cases.BN_REG1024X4
    table = [
        # fewer than 512 rows: the 1 024-thread form up to 1 024 x 4 x 4 floats, nothing between it and the generic kernel ...
        (1, 4, w), (511, 16384, w), (511, 16388, g), (511, 16380, w), (1, 16384, w),
        # ... from 512 rows on: 256 threads, 4 float4 up to 4 096, 12 float4 up to 12 288
        (512, 4, r4), (512, 4096, r4), (512, 4100, r12), (512, 12288, r12), (512, 12292, g), (512, 16384, g), (1024, 320, r4), (100000, 4096, r4),
        # N % 4 != 0: generic, whatever the size
        (3, 1, g), (3, 2, g), (3, 3, g), (3, 5, g), (511, 4097, g), (512, 4098, g), (512, 12287, g),
    ]
    _check(lib, "bn_rows", table)


def test_chan_layernorm_and_head_thresholds_from_both_sides(lib):
    table = [(64, 4, 1), (128, 4, 2), (1024, 4, 16), (64, 10240, 1), (128, 10240, 2), (1024, 10240, 16)]
    table += [(c, 32, 0) for c in (1, 32, 60, 63, 65, 68, 127, 129, 192, 256, 512, 960, 1023, 1025, 1088, 2048)]
    table += [(c, n, 0) for c in (64, 128, 1024) for n in (1, 2, 3, 5, 6, 7, 33, 34, 35)]
    _check(lib, "chan_layernorm", table)
    head = [(1024, 4, 1), (1024, 10240, 1)] + [(c, 32, 0) for c in (64, 128, 512, 960, 1023, 1025, 1088, 2048)] + [(1024, n, 0) for n in (1, 2, 3, 5, 6, 7, 570)]
    _check(lib, "head_ln_fc", head)


def test_dwconv_t_threshold_from_both_sides(lib):
    _check(lib, "dwconv_t", [(t, 1 if t % 4 == 0 else 0) for t in range(1, 70)])
