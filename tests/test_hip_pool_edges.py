"""The pooling kernels (csrc/pool.hip) and the 8x8 head at their edges: exact, element by element, with poisoned surroundings.

  advhip_maxpool3d_strided_f32 / advhip_maxpool3d_padded_f32 on the cases of tests/pool_cases.py (the smallest shapes that reach each
      edge of the wave-per-row, the temporal and the generic kernel; the table there says what each is for), on one sample per input
      position with a NaN / a +1000 at that position, with y a channel slice of a wider sentinel tensor, with x on a 4-byte boundary,
      and once past the first sweep of either grid-stride loop
  advhip_global_avgpool_f32 on every n of {1, 2, 63, 64, 65, 98, 127, 128, 129, 191, 192, 193, 4097} x {1, 3, 4, 5, 9} rows
  I3D8x8R50.head (the weights of _head_weights + ops.bgemm, as forward runs them) on five feature-map sizes

Max pooling selects, so the result must be the reference of tests/_pool_ref.py bit for bit (R.differs: the same NaN positions, == elsewhere;
zeros of either sign are equal).  The mean's inputs are integers / 4 whose every partial sum is exact in fp32, and the kernel ends in
one IEEE division: the result must EQUAL float32(sum / n).  Real-valued rows and the head are held to derived bounds (stated at the
tests).  Inputs are views with at least 1 024 NaN floats on either side inside the same allocation, outputs views into sentinel-filled
ones; after every launch the input allocation and the output's surroundings are compared bit for bit with what was handed over.  For
every launch there are two outcomes: the refusal the launcher documents (tests/_pool_ref.py: expected_refusal), or the reference.

test_every_form_was_reached reads what the tests above it recorded (selected on its own, it runs one parameter set of each first) and
prints the counts (`pytest -s`).

Measured on an MI355X (printed by test_every_form_was_reached on every run): the 60 tests of this file take 3.6 s, 1.4 s of it between
the first test and the last; 190 launches, all 190 returned the reference, and 3 refusals, each with the documented text.  The largest
error over its bound: 0.002 (real-valued mean), 0.004 (head).
"""
import math
import re
import time

import pytest
import torch

import _pool_ref as R
import pool_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = -12345.0
GUARD = 1024  # floats of NaN / sentinel on either side of every operand, inside its allocation

RAN = set()      # (query, form) of every launch that returned the reference
REFUSED = set()  # the documented texts seen
COUNT = {"launches": 0, "references": 0, "refusals": 0}
CLOCK = {}


def _mods():
    from anomaly_detection_on_video_amd import _lib, ops

    return _lib, ops


@pytest.fixture(autouse=True, scope="module")
def _clock():
    CLOCK["start"] = time.perf_counter()
    yield


def _bits(t):
    return t.view(torch.int32)


class Guarded:
    """A tensor on the device inside a larger `fill`-filled allocation: `view` (dense, `offset` floats past a 16-byte boundary, or a
    channel slice [lo, lo + c) of a wider NCDHW tensor that is itself `fill`), the allocation as it was handed over, and the flat
    indices of everything but the view"""

    def __init__(self, t, fill, offset=0, wide=0, lo=0):
        if wide:
            full = torch.full((t.shape[0], t.shape[1] + wide) + tuple(t.shape[2:]), fill, dtype=t.dtype)
            full[:, lo : lo + t.shape[1]] = t
            v = R.embed(full, GUARD, fill, offset, device=DEV)[:, lo : lo + t.shape[1]]
        else:
            v = R.embed(t, GUARD, fill, offset, device=DEV)
        self.view, self.base = v, v._base
        self.geom = (tuple(v.shape), tuple(v.stride()), v.storage_offset())
        self.pristine = self.base.clone()
        self.outside = R.outside(torch.arange(self.base.numel(), device=DEV).as_strided(*self.geom))  # (of the indices: the indices outside)
        assert self.outside.numel() >= 2 * GUARD and self.outside.numel() + v.numel() == self.base.numel()

    def fresh(self):
        """a new allocation with the same content -> (view, base)"""
        b = self.pristine.clone()
        return b.as_strided(*self.geom), b

    def changed(self):
        """0-dim bool tensor: some bit of the allocation differs from what was handed over"""
        return (_bits(self.base) != _bits(self.pristine)).any()

    def outside_changed(self, base):
        return (_bits(base).index_select(0, self.outside) != _bits(self.pristine).index_select(0, self.outside)).any()


def _sentinel(shape, **kw):
    return Guarded(torch.full(tuple(shape), SENT), SENT, **kw)


def _report(bad):
    assert not bad, f"{len(bad)} complaints, the first 20:\n" + "\n".join(bad[:20])


# ---- max pooling -------------------------------------------------------------------------------------------------------------------------
def _launch_maxpool(x, y, k, s, p=None):
    """the C entry point on test-owned buffers: y dense, or a channel slice (its batch stride is handed over as it is)"""
    _lib, ops = _mods()
    lib = _lib.load()
    b, c, t, h, w = x.shape
    assert x.is_contiguous() and x.dtype == y.dtype == torch.float32
    if p is None:
        ybs = 0 if y.is_contiguous() else y.stride(0)
        _lib.check(lib.advhip_maxpool3d_strided_f32(_lib.ptr(x), _lib.ptr(y), ybs, b, c, t, h, w, *k, *s, _lib.stream()), "maxpool3d")
        return ybs
    assert y.is_contiguous()
    _lib.check(lib.advhip_maxpool3d_padded_f32(_lib.ptr(x), _lib.ptr(y), b, c, t, h, w, *k, *s, *p, _lib.stream()), "maxpool3d_padded")
    return 0


class Pending:
    """The launches of one test: everything is judged after one synchronisation"""

    def __init__(self):
        self.items, self.bad, self.refused = [], [], []  # (refused: the documented texts this test's launches were refused with)

    def maxpool(self, what, xg, want, og, k, s, p=None, form=None, also=None):
        """One launch of x = xg.view into a fresh copy of og -> the output view (or None: refused as documented).  `form`: the kernel
        the case is there for, checked against the library's answer for THIS launch; `also`: a tensor the result must equal as well."""
        _lib, ops = _mods()
        out, out_base = og.fresh()
        ybs = 0 if out.is_contiguous() else out.stride(0)
        refusal = R.expected_refusal(tuple(xg.view.shape), k, s, p, ybs)
        if p is None:
            padded_y = ybs != 0 and ybs != out.shape[1] * math.prod(out.shape[2:])
            asked = cases.maxpool_form(_lib.load(), xg.view.shape, k, s, padded_y)
        else:
            asked = cases.GENERIC
        if form is not None and asked != form:
            self.bad.append(f"{what}: the library answers form {asked}, the case is listed with {form}")
        try:
            _launch_maxpool(xg.view, out, k, s, p)
        except _lib.HipExtensionError as e:
            COUNT["refusals"] += 1
            if refusal is None or not re.search(refusal, str(e)):
                self.bad.append(f"{what}: refused with '{e}', expected {'a result' if refusal is None else repr(refusal)}")
            else:
                REFUSED.add(refusal)
                self.refused.append(refusal)
            # a refusal comes before any launch: the whole output allocation (the view is all SENT) and the input are as handed over
            if bool((_bits(out_base) != _bits(og.pristine)).any()) or bool((out != SENT).any()) or bool(xg.changed()):
                self.bad.append(f"{what}: refused, but the output allocation or the input changed")
            return None
        COUNT["launches"] += 1
        if refusal is not None:
            self.bad.append(f"{what}: ran, although the launcher documents '{refusal}'")
            return None
        wrong = R.differs(out, want).any()
        if also is not None:
            wrong = wrong | R.differs(out, also).any()
        self.items.append((what, ("maxpool3d", asked), out, want, torch.stack([wrong, og.outside_changed(out_base), xg.changed()])))
        return out

    def add(self, what, key, out, want, flags):
        self.items.append((what, key, out, want, torch.stack(flags)))

    def judge(self):
        flags = torch.stack([i[4] for i in self.items]).cpu().tolist() if self.items else []
        for (wrong, sentinel, xbad), (what, key, out, want, _f) in zip(flags, self.items):
            if wrong:
                self.bad.append(f"{what}: " + R.describe(out, want))
            if sentinel:
                self.bad.append(f"{what}: the surroundings of the output changed")
            if xbad:
                self.bad.append(f"{what}: the input or its surroundings changed")
            if not (wrong or sentinel or xbad):
                RAN.add(key)
                COUNT["references"] += 1
        _report(self.bad)


def _maxpool_case(pend, name, shape, k, s, p, form):
    for nan in (0.0, 0.03):
        x = R.values(f"edges.{name}", shape, k=R.corner(shape, k, s, p), nan=nan)
        want = R.maxpool_ref(x, k, s, p if p is not None else (0, 0, 0)).to(DEV)
        pend.maxpool(f"{name} {shape} k{k} s{s} p{p} NaN {nan}", Guarded(x, NAN), want, _sentinel(want.shape), k, s, p, form)


@pytest.mark.parametrize("case", cases.MAXPOOL_CASES, ids=[c[0] for c in cases.MAXPOOL_CASES])
def test_maxpool_equals_the_reference(case):
    """Random fp32 mixed with denormals, +-inf, ties and a window that is all -inf, then the same with 3 % NaN: the reference, element by
    element, on the kernel the case is listed with."""
    name, shape, k, s, form = case
    pend = Pending()
    _maxpool_case(pend, name, shape, k, s, None, form)
    pend.judge()


def test_padded_maxpool_equals_the_reference():
    """advhip_maxpool3d_padded_f32: the 8x8 stem pool k(1,3,3) s(1,2,2) p(0,1,1) on every H, W of {1, 2, 3, 7, 8}, k(3,3,3) on one frame,
    and padding of exactly half the window."""
    pend = Pending()
    for name, shape, k, s, p in cases.PADDED_CASES:
        _maxpool_case(pend, name, shape, k, s, p, cases.GENERIC)
    pend.judge()


@pytest.mark.parametrize("sweep", cases.SWEEPS, ids=[c[0] for c in cases.SWEEPS])
def test_one_value_at_every_position_lands_in_exactly_its_windows(sweep):
    """Sample i is a random background with a NaN -- then with +1000 -- at flat input position i; one launch per value.  The result is
    the reference, and, stated without the reference: the value appears in exactly the outputs whose window holds position i (in none,
    for the column, row or frame that no window reads), be it the window's first, second or third column."""
    name, thw, k, s, p, form = sweep
    n = thw[0] * thw[1] * thw[2]
    dims = R.out_dims(thw, k, s, p)
    holds = torch.zeros((n, 1) + dims, dtype=torch.bool)
    for i in range(n):
        pos = (i // (thw[1] * thw[2]), i // thw[2] % thw[1], i % thw[2])
        for o in R.windows_holding(thw, k, s, p, pos):
            holds[(i, 0) + o] = True
    unread = int((holds.reshape(n, -1).sum(dim=1) == 0).sum())
    if name.startswith("sweep.233"):
        assert unread > 0  # the last column (and row, and frame) of these geometries
    holds = holds.to(DEV)
    pend = Pending()
    outs = {}
    for label, value in (("NaN", NAN), ("+1000", 1000.0)):
        x = R.sweep_input(name, thw, value)
        want = R.maxpool_ref(x, k, s, p).to(DEV)
        outs[label] = pend.maxpool(f"{name} {thw} {label}", Guarded(x, NAN), want, _sentinel(want.shape), k, s, p if any(p) else None, form)
    pend.judge()
    assert bool((torch.isnan(outs["NaN"]) == holds).all()), f"{name}: a NaN outside the windows that hold it, or missing from one"
    assert bool(((outs["+1000"] == 1000.0) == holds).all()), f"{name}: +1000 outside the windows that hold it, or missing from one"
    print(f"{name}: {n} positions, {unread} of them read by no window")


def test_y_as_a_channel_slice_equals_the_dense_call():
    """y = channels [3, 3 + C) of C + 5 of a sentinel tensor, B = 2: the wave-per-row kernel's edge shapes, a temporal shape (which must
    fall to the generic kernel) and a generic one.  The reference, the dense call's result, and every sentinel untouched."""
    pend = Pending()
    for name, form in cases.YSLICE_CASES:
        _n, shape, k, s, dense_form = cases.MAXPOOL_CASE[name]
        shape = (cases.YSLICE_B,) + tuple(shape[1:])
        x = R.values(f"yslice.{name}", shape, k=R.corner(shape, k, s), nan=0.02)
        want = R.maxpool_ref(x, k, s).to(DEV)
        xg = Guarded(x, NAN)
        dense = pend.maxpool(f"{name} {shape} dense", xg, want, _sentinel(want.shape), k, s, None, dense_form)
        og = _sentinel(want.shape, wide=cases.YSLICE_WIDE, lo=cases.YSLICE_LO)
        assert not og.view.is_contiguous() and og.view.stride(0) == (shape[1] + cases.YSLICE_WIDE) * math.prod(want.shape[2:])
        pend.maxpool(f"{name} {shape} y a channel slice", xg, want, og, k, s, None, form, also=dense)
    pend.judge()


def test_x_on_a_4_byte_boundary():
    """x one float past a 16-byte boundary: the wave-per-row kernel's float2 loads sit on 4-byte addresses, which gfx950 allows and the
    launcher does not look at."""
    pend = Pending()
    for name, form in cases.OFF1_CASES:
        _n, shape, k, s, _f = cases.MAXPOOL_CASE[name]
        x = R.values(f"off1.{name}", shape, k=R.corner(shape, k, s), nan=0.02)
        want = R.maxpool_ref(x, k, s).to(DEV)
        xg = Guarded(x, NAN, offset=1)
        assert xg.view.data_ptr() % 8 == 4
        pend.maxpool(f"{name} {shape} x off by one float", xg, want, _sentinel(want.shape), k, s, None, form)
    pend.judge()


@pytest.mark.parametrize("case", cases.GRID_CASES, ids=[c[0] for c in cases.GRID_CASES])
def test_grid_stride_loop_goes_round_twice(case):
    """The smallest totals past one sweep of the generic kernel's grid (8 192 x 256) and of the temporal kernel's (4 096 x 256 x 4
    unrolled): the outputs past the first sweep are compared like all others."""
    name, shape, k, s, form, outputs, sweep = case
    x = R.big_values(len(name), shape)
    xg = Guarded(x, NAN)
    want = R.maxpool_ref(xg.view, k, s)  # the same plain reference, run on the device
    assert want.numel() == outputs > sweep
    pend = Pending()
    out = pend.maxpool(f"{name} {shape}", xg, want, _sentinel(want.shape), k, s, None, form)
    pend.judge()
    assert not bool(R.differs(out.reshape(-1)[sweep:], want.reshape(-1)[sweep:]).any()) and not bool((out.reshape(-1)[sweep:] == SENT).any())


def test_launches_that_must_be_refused_are_refused_on_the_device_too():
    """T < kt, a y batch stride below one sample, padding of more than half the window -- with real buffers: the documented text, and
    nothing written."""
    pend = Pending()
    x = R.values("refused", (2, 3, 2, 5, 8))
    xg = Guarded(x, NAN)
    assert pend.maxpool("T < kt", xg, None, _sentinel((2, 3, 1, 2, 3)), (3, 3, 3), cases.S222) is None
    og = _sentinel((2, 3, 1, 2, 3), wide=5, lo=3)
    short = og.view.as_strided(og.view.shape, (17,) + tuple(og.view.stride()[1:]), og.view.storage_offset())
    _lib, _ops = _mods()
    with pytest.raises(_lib.HipExtensionError, match=r"y batch stride 17 < one sample \(18\)"):
        _launch_maxpool(xg.view, short, cases.K233, cases.S222)
    COUNT["refusals"] += 1
    assert pend.maxpool("padding above half", xg, None, _sentinel((2, 3, 2, 4, 4)), (1, 3, 3), (1, 2, 2), (0, 2, 1)) is None
    _report(pend.bad)  # (a refused launch that left its output allocation or its input changed is a complaint of pend.maxpool)
    assert pend.refused == [R.expected_refusal((2, 3, 2, 5, 8), (3, 3, 3), cases.S222), R.expected_refusal((2, 3, 2, 5, 8), (1, 3, 3), (1, 2, 2), (0, 2, 1))]
    assert None not in pend.refused and not bool(og.changed()) and not bool(xg.changed())


# ---- the mean ----------------------------------------------------------------------------------------------------------------------------
def _launch_mean(x, y):
    _lib, ops = _mods()
    rows, n = x.shape
    assert x.is_contiguous() and y.is_contiguous() and y.numel() == rows
    _lib.check(_lib.load().advhip_global_avgpool_f32(_lib.ptr(x), _lib.ptr(y), rows, n, _lib.stream()), "global_avgpool")
    COUNT["launches"] += 1


def _mean(pend, what, x, want, n):
    _lib, ops = _mods()
    xg, og = Guarded(x, NAN), _sentinel((x.shape[0],))
    out, out_base = og.fresh()
    _launch_mean(xg.view, out)
    want = want.to(DEV)
    form = cases.avgpool_form(_lib.load(), n)
    pend.add(what, ("global_avgpool", form), out, want, [R.differs(out, want).any(), og.outside_changed(out_base), xg.changed()])
    return out


@pytest.mark.parametrize("n", cases.MEAN_N)
def test_mean_of_exactly_summable_rows_is_the_rounded_quotient(n):
    """Integers in [-256, 256] / 4: every partial sum, in any order, is exact in fp32, and both of the kernel's divisions are IEEE ones:
    the result EQUALS float32(fp64 sum / n) and fp32(sum) / fp32(n).  Rows 1, 3, 4, 5, 9: whole and partial workgroups of four waves.  A
    read of p[n] meets the next row, or the NaN behind the last one."""
    assert cases.mean_form(n) == (1 if n <= 128 else 0)
    pend = Pending()
    for rows in cases.MEAN_ROWS:
        x = R.quarters(f"mean.{n}.{rows}", (rows, n))
        want = R.mean_ref(x)
        assert torch.equal(want, x.sum(dim=1) / torch.tensor(float(n))) and torch.equal(x.sum(dim=1).double(), x.double().sum(dim=1))
        _mean(pend, f"mean n {n} rows {rows}", x, want, n)
    pend.judge()


@pytest.mark.parametrize("n", cases.MEAN_N)
def test_mean_of_a_non_finite_row(n):
    """One NaN, then one +inf, then +inf together with -inf, in turn at the first, the 64th and the last position of a row (those that
    the row has): the row gives NaN / +inf / NaN; the rows between them -- every second row is clean -- keep their exact mean."""
    scen = [(kind, pos) for kind in ("nan", "inf", "pair") for pos in sorted({0, 63, n - 1}) if pos < n and (kind != "pair" or n > 1)]
    rows = 2 * len(scen) + 1
    clean = R.quarters(f"mean.nonfinite.{n}", (rows, n))
    x = clean.clone()
    expect = R.mean_ref(clean)
    for j, (kind, pos) in enumerate(scen):
        r = 2 * j + 1
        x[r, pos] = NAN if kind == "nan" else math.inf
        if kind == "pair":
            x[r, (pos + 1) % n] = -math.inf
        expect[r] = math.inf if kind == "inf" else NAN
    want = R.mean_ref(x)
    assert not bool(R.differs(want, expect).any())  # what the reference gives is what the test's docstring says
    pend = Pending()
    _mean(pend, f"mean n {n} non-finite rows", x, want, n)
    pend.judge()


@pytest.mark.parametrize("n", cases.MEAN_REAL_N)
def test_mean_of_real_rows_within_the_summation_bound(n):
    """Real values of both signs against fp64: |error| <= n 2^-23 mean|x| per row -- any-order fp32 summation of n terms errs by at most
    (n - 1) 2^-24 sum|x| to first order, the division by half an ulp more: n 2^-24 sum|x| / n = 2^-24 sum|x|, so this bound (= 2^-23
    sum|x|) leaves a factor 2."""
    _lib, ops = _mods()
    x = R.mixed(f"mean.real.{n}", (9, n))
    assert bool((x < 0).any()) and bool((x > 0).any())
    xg, og = Guarded(x, NAN), _sentinel((9,))
    out, out_base = og.fresh()
    _launch_mean(xg.view, out)
    err = (out.cpu().double() - R.mean_ref64(x)).abs()
    bound = n * 2.0 ** -23 * x.double().abs().mean(dim=1)
    print(f"mean n {n}: largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (n, float((err / bound).max()))
    assert not bool(og.outside_changed(out_base)) and not bool(xg.changed())
    RAN.add(("global_avgpool", cases.avgpool_form(_lib.load(), n)))
    COUNT["references"] += 1


# ---- the 8x8 head ------------------------------------------------------------------------------------------------------------------------
_MODEL = []


def _model():
    """one I3D8x8R50; the head uses none of its parameters, which stay on the host"""
    if not _MODEL:
        from anomaly_detection_on_video_amd.i3d_ptv import I3D8x8R50

        _MODEL.append(I3D8x8R50())
    return _MODEL[0]


@pytest.mark.parametrize("thw", cases.HEAD_GEOMETRIES, ids=str)
def test_head_equals_torchs_two_average_pools(thw):
    """I3D8x8R50.head -- _head_weights + ops.bgemm, the two lines forward runs -- on (2, 65, T, H, W) of both signs against
    AvgPool3d((4,7,7), 1) + the mean in fp64.  Per row |error| <= (K + 2) 2^-23 sum_i |w_i x_i|, K = T H W: an fp32 dot product of K
    terms errs by at most K 2^-24 sum|w x| to first order in any order, the weights' own rounding to fp32 adds 2^-24 sum|w x|; twice that."""
    from anomaly_detection_on_video_amd.i3d_ptv import HEAD_POOL, I3D8x8R50

    assert tuple(HEAD_POOL) == R.HEAD_POOL  # head_ref pools over the window the model names
    b, c = cases.HEAD_BC
    x = R.mixed(f"head.{thw}", (b, c) + tuple(thw))
    rows = x.reshape(b * c, -1)
    assert bool(((rows < 0).any(dim=1) & (rows > 0).any(dim=1)).all())  # no row is all-positive
    xg = Guarded(x, NAN)
    got = _model().head(xg.view)
    COUNT["launches"] += 1
    assert tuple(got.shape) == (b, c, 1, 1, 1)
    want = R.head_ref(x)
    k = rows.shape[1]
    w = I3D8x8R50._head_weights_f64(tuple(thw)).reshape(1, -1)
    bound = (k + 2) * 2.0 ** -23 * (w * rows.double().abs()).sum(dim=1)
    err = (got.cpu().double().reshape(-1) - want.reshape(-1)).abs()
    print(f"head {thw}: largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (thw, float((err / bound).max()))
    assert not bool(xg.changed())
    COUNT["references"] += 1
    RAN.add(("head", tuple(thw)))


@pytest.mark.parametrize("thw", cases.HEAD_TOO_SMALL, ids=str)
def test_head_refuses_a_map_smaller_than_its_window(thw):
    with pytest.raises(ValueError, match="smaller than the head's AvgPool3d"):
        _model().head(torch.zeros((1, 2) + tuple(thw), device=DEV))


# ---- what all of the above covered ---------------------------------------------------------------------------------------------------------
def test_every_form_was_reached():
    """What the tests above recorded: every form of both queries was reached by at least one launch that returned the reference."""
    # selected on its own, with -k, or run before the others: a form nothing has reached yet gets one case of its own first
    stand_in = {("maxpool3d", cases.ROW233): lambda: test_maxpool_equals_the_reference(cases.MAXPOOL_CASE["233.rows5"]),
                ("maxpool3d", cases.TEMPORAL): lambda: test_maxpool_equals_the_reference(cases.MAXPOOL_CASE["t.five"]),
                ("maxpool3d", cases.GENERIC): lambda: test_maxpool_equals_the_reference(cases.MAXPOOL_CASE["g.k122"]),
                ("global_avgpool", cases.AVG_BUTTERFLY): lambda: test_mean_of_exactly_summable_rows_is_the_rounded_quotient(128),
                ("global_avgpool", cases.AVG_STRIDED): lambda: test_mean_of_exactly_summable_rows_is_the_rounded_quotient(129)}
    for form in cases.ALL_FORMS:
        if form not in RAN:
            stand_in[form]()
    torch.cuda.synchronize()
    print(f"launches / references returned / refusals: {COUNT}; {time.perf_counter() - CLOCK['start']:.1f} s since the file's first test")
    print("refusals seen:", sorted(REFUSED))
    print("forms reached:", sorted(k for k in RAN if k[0] != "head"), "head geometries:", sorted(k[1] for k in RAN if k[0] == "head"))
    missing = [f for f in cases.ALL_FORMS if f not in RAN]
    assert not missing, f"no launch that returned the reference reached {missing}"
    assert COUNT["references"] > 0 and COUNT["references"] <= COUNT["launches"]
