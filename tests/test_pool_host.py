"""CPU-only: the pooling launchers' choice of kernel (csrc/pool.hip) through the library's form queries -- the rule the launcher
itself calls -- their refusals through the raw C ABI, the reference of tests/_pool_ref.py against torch on every case the GPU file
runs, and the 8x8 head's weights restated against torch's AvgPool3d in fp64.  If a threshold moves, this fails instead of the GPU
cases of tests/test_hip_pool_edges.py quietly running another kernel."""
import ctypes as C
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _pool_ref as R
import pool_cases as cases
from conftest import REPO

QUERIES = ("advhip_maxpool3d_form", "advhip_global_avgpool_form")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    return _lib.load()


# ---- the reference against torch ------------------------------------------------------------------------------------------------------
def _every_maxpool_case():
    """(input name, shape, k, s, p, NaN fractions) of everything the GPU file launches, under the names it makes its inputs with -- the
    same tensors -- the grid-stride shapes excepted (their reference is the same code, run on the device) and the sweep geometries on
    random values here (their own inputs: test_sweep_inputs_put_one_value_at_each_position)"""
    for name, shape, k, s, _form in cases.MAXPOOL_CASES:
        yield f"edges.{name}", shape, k, s, (0, 0, 0), (0.0, 0.03)
    for name, shape, k, s, p in cases.PADDED_CASES:
        yield f"edges.{name}", shape, k, s, p, (0.0, 0.03)
    for name, _form in cases.YSLICE_CASES:
        _n, shape, k, s, _f = cases.MAXPOOL_CASE[name]
        yield f"yslice.{name}", (cases.YSLICE_B,) + tuple(shape[1:]), k, s, (0, 0, 0), (0.02,)
    for name, _form in cases.OFF1_CASES:
        _n, shape, k, s, _f = cases.MAXPOOL_CASE[name]
        yield f"off1.{name}", shape, k, s, (0, 0, 0), (0.02,)
    for name, thw, k, s, p, _form in cases.SWEEPS:
        yield f"host.{name}", (2, 1) + tuple(thw), k, s, p, (0.0, 0.03)


def test_maxpool_ref_equals_torch_on_every_case():
    """Under the comparison rule (the same NaN positions, == elsewhere), with and without NaN among the inputs; the inputs hold +-inf,
    denormals, ties, zeros of both signs and a first window that is all -inf."""
    seen = {"nan": 0, "+inf": 0, "-inf": 0, "denormal": 0}
    for name, shape, k, s, p, nans in _every_maxpool_case():
        for nan in nans:
            corner = R.corner(shape, k, s, p)
            x = R.values(name, shape, k=corner, nan=nan)
            want = F.max_pool3d(x, k, s, p)
            got = R.maxpool_ref(x, k, s, p)
            assert got.shape == want.shape and got.dtype == torch.float32, name
            assert not bool(R.differs(got, want).any()), f"{name} nan {nan}: " + R.describe(got, want)
            assert corner is None or float(got[0, 0, 0, 0, 0]) == -math.inf, name  # the window that holds nothing but -inf
            seen["nan"] += int(torch.isnan(got).sum())
            seen["+inf"] += int((got == math.inf).sum())
            seen["-inf"] += int((got == -math.inf).sum())
            seen["denormal"] += int(((got != 0) & (got.abs() < 2.0 ** -126)).sum())
    assert all(v > 0 for v in seen.values()), seen  # every kind reaches some OUTPUT, not only the inputs


def test_sweep_inputs_put_one_value_at_each_position():
    for name, thw, k, s, p, _form in cases.SWEEPS:
        n = thw[0] * thw[1] * thw[2]
        x = R.sweep_input(name, thw, float("nan"))
        assert x.shape == (n, 1) + tuple(thw)
        assert torch.equal(torch.isnan(x).reshape(n, n), torch.eye(n, dtype=torch.bool))
        got, want = R.maxpool_ref(x, k, s, p), F.max_pool3d(x, k, s, p)
        assert not bool(R.differs(got, want).any()), name
        # windows_holding, which the GPU file's sweep argues with, agrees with where the reference puts the NaN
        dims = R.out_dims(thw, k, s, p)
        for i in range(n):
            pos = (i // (thw[1] * thw[2]), i // thw[2] % thw[1], i % thw[2])
            hit = {tuple(int(v) for v in idx) for idx in torch.isnan(got[i, 0]).nonzero().tolist()}
            assert hit == R.windows_holding(thw, k, s, p, pos), (name, pos)
        assert dims == tuple(got.shape[2:])


def test_mean_ref_is_the_rounded_quotient_and_quarters_sum_exactly():
    for n in cases.MEAN_N:
        x = R.quarters(f"mean.{n}", (9, n))
        assert float(x.abs().max()) <= 64.0 and torch.equal(x * 4.0, (x * 4.0).round())
        s32 = x.sum(dim=1)  # fp32, torch's own order
        s64 = x.double().sum(dim=1)
        assert torch.equal(s32.double(), s64), n
        assert torch.equal(R.mean_ref(x), s32 / torch.tensor(float(n))), n  # fp32(sum) / fp32(n), one IEEE division
    x = R.mixed("mean.real", (5, 200))
    assert bool((x < 0).any()) and bool((x > 0).any())


# ---- the queries ----------------------------------------------------------------------------------------------------------------------
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
    for macro, value in (("GENERIC", cases.GENERIC), ("ROW233", cases.ROW233), ("TEMPORAL", cases.TEMPORAL)):
        assert re.search(rf"#define\s+ADVHIP_MAXPOOL_{macro}\s+{value}\b", text), macro
    assert (_lib.MAXPOOL_GENERIC, _lib.MAXPOOL_ROW233, _lib.MAXPOOL_TEMPORAL) == (0, 1, 2)


def test_every_gpu_case_takes_the_form_it_is_listed_with(lib):
    reached = set()
    for name, shape, k, s, form in cases.MAXPOOL_CASES:
        assert cases.maxpool_form(lib, shape, k, s, False) == form, name
        reached.add(("maxpool3d", form))
    for name, thw, k, s, p, form in cases.SWEEPS:
        if not any(p):
            assert cases.maxpool_form(lib, thw, k, s, False) == form, name
        else:
            assert form == cases.GENERIC, name  # the padded entry point has the generic kernel only
    for name, form in cases.YSLICE_CASES:
        _n, shape, k, s, dense_form = cases.MAXPOOL_CASE[name]
        assert cases.maxpool_form(lib, shape, k, s, True) == form, name
        assert form == (dense_form if dense_form != cases.TEMPORAL else cases.GENERIC), name
    assert {cases.MAXPOOL_CASE[n][4] for n, _f in cases.YSLICE_CASES} == {cases.GENERIC, cases.ROW233, cases.TEMPORAL}
    assert [n for n, _f in cases.YSLICE_CASES][:4] == [c[0] for c in cases.MAXPOOL_CASES[:4]]  # the first four 233 rows of the table
    for name, form in cases.OFF1_CASES:
        _n, shape, k, s, dense_form = cases.MAXPOOL_CASE[name]
        assert cases.maxpool_form(lib, shape, k, s, False) == form == dense_form, name
    assert {f for _n, f in cases.OFF1_CASES} == {cases.ROW233, cases.TEMPORAL}
    for name, shape, k, s, form, outputs, sweep in cases.GRID_CASES:
        assert cases.maxpool_form(lib, shape, k, s, False) == form, name
        b, c, t, h, w = shape
        to, ho, wo = R.out_dims((t, h, w), k, s)
        assert b * c * to * ho * wo == outputs and sweep < outputs < sweep + sweep // 64, name  # just past one sweep of the grid
    for n in cases.MEAN_N + cases.MEAN_REAL_N:
        assert cases.avgpool_form(lib, n) == cases.mean_form(n), n
        reached.add(("global_avgpool", cases.mean_form(n)))
    assert {cases.mean_form(n) for n in cases.MEAN_REAL_N} == {cases.AVG_STRIDED, cases.AVG_BUTTERFLY}
    assert reached == set(cases.ALL_FORMS)


def test_thresholds_from_both_sides(lib):
    g, r, t = cases.GENERIC, cases.ROW233, cases.TEMPORAL
    k, s = cases.K233, cases.S222

    def form(w, k, s, padded=False):
        return cases.maxpool_form(lib, (w,), k, s, padded)

    for w in (4, 126, 128):
        assert form(w, k, s) == r, w
    for w in (127, 129, 130):
        assert form(w, k, s) == g, w
    for w in (3, 5, 125, 132, 256):
        assert form(w, k, s) == g, w
    for w in range(4, 129, 2):
        assert form(w, k, s) == r, w
    assert form(64, k, (2, 2, 1)) == g
    # every other window or stride one step away from (2,3,3) / (2,2,2)
    for kk, ss in (((1, 3, 3), s), ((3, 3, 3), s), ((2, 2, 3), s), ((2, 3, 2), s), ((2, 3, 4), s), (k, (1, 2, 2)), (k, (2, 1, 2)), (k, (2, 3, 2)), (k, (2, 2, 3))):
        assert form(64, kk, ss) == g, (kk, ss)
    # y padded between samples changes nothing for the wave-per-row kernel, which adds the padding per sample ...
    for w in (4, 126, 128):
        assert form(w, k, s, True) == r, w
    for w in (127, 129, 130):
        assert form(w, k, s, True) == g, w
    # ... and sends a temporal pool to the generic kernel, the only other one that does
    for kt, st in ((2, 2), (3, 2), (2, 1), (5, 3)):
        assert form(55, (kt, 1, 1), (st, 1, 1)) == t, (kt, st)
        assert form(55, (kt, 1, 1), (st, 1, 1), True) == g, (kt, st)
    for kk, ss in (((2, 2, 1), (2, 1, 1)), ((2, 1, 2), (2, 1, 1)), ((2, 1, 1), (2, 2, 1)), ((2, 1, 1), (2, 1, 2))):
        assert form(55, kk, ss) == g, (kk, ss)
    assert form(55, (1, 1, 1), (1, 1, 1)) == t  # the identity pool is a temporal one
    assert (cases.avgpool_form(lib, 128), cases.avgpool_form(lib, 129)) == (1, 0)
    for n in range(1, 129):
        assert cases.avgpool_form(lib, n) == 1, n
    for n in (130, 191, 4097, 2 ** 31 - 1):
        assert cases.avgpool_form(lib, n) == 0, n


# ---- the refusals, through the raw C ABI (nothing is launched: the pointers are never read) ----------------------------------------
def test_refusals_return_einval_with_the_documented_text(lib):
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)

    def refused(rc, text):
        assert rc == EINVAL, (rc, text)
        msg = lib.advhip_last_error().decode()
        assert re.search(text, msg), (msg, text)

    dense = (1, 1, 2, 3, 4) + cases.K233 + cases.S222
    for x, y in ((None, p), (p, None)):
        refused(lib.advhip_maxpool3d_f32(x, y, *dense, None), r"^maxpool3d: null pointer$")
        refused(lib.advhip_maxpool3d_strided_f32(x, y, 0, *dense, None), r"^maxpool3d: null pointer$")
        refused(lib.advhip_maxpool3d_padded_f32(x, y, *dense, 0, 1, 1, None), r"^maxpool3d_padded: null pointer$")
        refused(lib.advhip_global_avgpool_f32(x, y, 4, 98, None), r"^global_avgpool: bad arguments$")
    # T < kt (and H < kh, W < kw, B = 0)
    for b, t, h, w in ((1, 1, 3, 4), (1, 2, 2, 4), (1, 2, 3, 2), (0, 2, 3, 4)):
        refused(lib.advhip_maxpool3d_f32(p, p, b, 1, t, h, w, *cases.K233, *cases.S222, None),
                rf"^maxpool3d: bad shape \(B={b} C=1 T={t} H={h} W={w} k=2,3,3 s=2,2,2\)$")
    refused(lib.advhip_maxpool3d_strided_f32(p, p, 0, 1, 1, 1, 5, 5, 2, 1, 1, 2, 1, 1, None), r"^maxpool3d: bad shape \(B=1 C=1 T=1 ")
    # padding more than half a window, along each axis
    for pad in ((1, 0, 0), (0, 2, 0), (0, 0, 2)):
        refused(lib.advhip_maxpool3d_padded_f32(p, p, 1, 1, 4, 5, 6, 1, 3, 3, 1, 2, 2, *pad, None),
                rf"^maxpool3d_padded: bad shape \(T=4 H=5 W=6 k=1,3,3 s=1,2,2 p={pad[0]},{pad[1]},{pad[2]}; padding at most half the window\)$")
    # T + 2 pt < kt: one frame, a 4-frame window, one frame of padding on either side
    refused(lib.advhip_maxpool3d_padded_f32(p, p, 1, 1, 1, 5, 6, 4, 3, 3, 2, 2, 2, 1, 1, 1, None),
            r"^maxpool3d_padded: bad shape \(T=1 H=5 W=6 k=4,3,3 s=2,2,2 p=1,1,1; padding at most half the window\)$")
    # a y batch stride below one sample: (1,3,2,5,8) -> 3 x 1 x 2 x 3 = 18 outputs per sample
    refused(lib.advhip_maxpool3d_strided_f32(p, p, 17, 2, 3, 2, 5, 8, *cases.K233, *cases.S222, None),
            r"^maxpool3d: y batch stride 17 < one sample \(18\)$")
    for rows, n in ((0, 98), (-1, 98), (4, 0), (4, -3)):
        refused(lib.advhip_global_avgpool_f32(p, p, rows, n, None), r"^global_avgpool: bad arguments$")


# ---- the 8x8 head's weights -------------------------------------------------------------------------------------------------------------
_MODEL = []


def _model():
    """one I3D8x8R50 (its parameters stay on the host and are never used)"""
    if not _MODEL:
        from anomaly_detection_on_video_amd.i3d_ptv import I3D8x8R50

        _MODEL.append(I3D8x8R50())
    return _MODEL[0]


@pytest.mark.parametrize("thw", cases.HEAD_HOST_GEOMETRIES, ids=str)
def test_head_weights_are_torchs_two_average_pools(thw):
    """Channel i of the identity is 1 at position i: head_ref of it is the weight torch's AvgPool3d((4,7,7), 1) + mean give that
    position.  _head_weights_f64 forms each weight with three divisions and two products (2.5 ulp), head_ref with one division and
    the sum of at most `windows` equal terms: |difference| <= (windows + 6) 2^-53 w.  The fp64 weights sum to 1 within 4 ulp
    (math.fsum adds them without error; 2.5 ulp relative on each is 1.25 ulp of the sum)."""
    from anomaly_detection_on_video_amd.i3d_ptv import HEAD_POOL, I3D8x8R50

    assert tuple(HEAD_POOL) == R.HEAD_POOL
    n = thw[0] * thw[1] * thw[2]
    w = I3D8x8R50._head_weights_f64(thw)
    assert w.dtype == torch.float64 and tuple(w.shape) == tuple(thw)
    want = R.head_ref(torch.eye(n, dtype=torch.float64).reshape((1, n) + tuple(thw))).reshape(thw)
    windows = math.prod(a - k + 1 for a, k in zip(thw, R.HEAD_POOL))
    excess = (w - want).abs() - (windows + 6) * 2.0 ** -53 * want
    assert float(excess.max()) <= 0.0, (thw, float((w - want).abs().max()))
    assert bool((w > 0).all())
    assert abs(math.fsum(w.reshape(-1).tolist()) - 1.0) <= 4 * 2.0 ** -52
    # the operand the GEMM gets is this, rounded once
    w32 = _model()._head_weights(tuple(thw), "cpu")
    assert w32.dtype == torch.float32 and tuple(w32.shape) == (n, 1) and torch.equal(w32.reshape(thw), w.float())


@pytest.mark.parametrize("thw", cases.HEAD_TOO_SMALL, ids=str)
def test_head_weights_refuse_a_map_smaller_than_the_window(thw):
    from anomaly_detection_on_video_amd.i3d_ptv import I3D8x8R50

    with pytest.raises(ValueError, match="smaller than the head's AvgPool3d"):
        I3D8x8R50._head_weights_f64(thw)
