"""The backbone's conv kernels at their window edges: exact, element by element, with poisoned surroundings.

  ops.conv3d_bn_act (advhip_conv3d_bn_act_ex_f32) on EVERY algorithm id the library accepts, the T-fold ids included, with the tile and
      the K slices pinned, on the geometry cases of tests/_conv3d_ref.py:

      name        Cin Cout kernel   stride   padding  (B,T,H,W)    what it exercises
      w33.s1        5   64 (1,3,3)  (1,1,1)  (0,1,1)  (2,2,7,9)    K = 45 (padded to 48 / 64); 126 positions per sample; M = 252: every BM has a
                                                                   partial last tile that straddles the samples
      w33.s2       16  128 (1,3,3)  (1,2,2)  (0,1,1)  (2,2,11,10)  stride 2 on an odd and an even extent; M = 120
      t3           64   64 (3,1,1)  (1,1,1)  (1,0,0)  (1,4,5,13)   M = 260 = 256 + 4; even T for TSPAN
      t3.T2        64  128 (3,1,1)  (1,1,1)  (1,0,0)  (2,2,7,7)    the T-fold's shape; 98-position rows
      t3.T1        32   64 (3,1,1)  (1,1,1)  (1,0,0)  (3,1,9,5)    T = 1: both outer taps are padding; T-fold at its smallest
      k1.s2        32  128 (1,1,1)  (1,2,2)  (0,0,0)  (2,2,9,11)   strided 1x1x1 (the downsample branch)
      k1.98        64  128 (1,1,1)  (1,1,1)  (0,0,0)  (3,2,7,7)    rows of 98: the virtual row padding to 100; three samples
      k1.257       64  128 (1,1,1)  (1,1,1)  (0,0,0)  (1,1,1,257)  M = 256 + 1; a row that is not a multiple of 4
      k1.260       64  128 (1,1,1)  (1,1,1)  (0,0,0)  (1,1,5,52)   M = 260, rows a multiple of 4: the 16-byte A path, MIXED and PERSIST
      stem          3   64 (5,7,7)  (2,2,2)  (2,3,3)  (2,5,11,13)  K = 735; every border class in t, h and w
      odd333        7   64 (3,3,3)  (1,2,1)  (1,0,2)  (1,3,5,7)    padding larger than k/2 along w, none along h; K = 189
      allpad       16   64 (3,3,3)  (1,1,1)  (1,1,1)  (2,1,1,1)    one output per sample; 26 of 27 taps in the padding
      k333.small   16   64 (3,3,3)  (1,1,1)  (1,1,1)  (1,2,2,3)    M = 12: every window touches every border

  the fused launches -- conv + (2,3,3) max-pool in its plain, column-parity and border-split forms, conv + (2,1,1) max-pool, conv + mean,
      the three uint8 stems -- against the fp64 conv + pool of tests/_conv3d_ref.py, not against another kernel of this library.

Integer operands and a BatchNorm whose fold is a power of two (tests/_conv3d_ref.py: assert_exact, called by every test here) make every
fp32 result exact for any summation order, tile or K split: results must EQUAL the reference.  Operands are views into NaN-filled
buffers (at least 1 024 floats on either side, inside the same allocation), outputs views into sentinel-filled ones; after every launch
the surroundings and the operands are compared bit for bit with what they held.  For every launch there are two outcomes: the refusal
the launcher documents (tests/_conv3d_ref.py: expected_refusal, written from include/advhip.h and the launchers' messages), or the reference.

test_every_family_met_every_edge reads what the tests above it recorded (selected on its own, it runs one parameter set of each first).

Measured on an MI355X (printed by test_every_family_met_every_edge on every run: `pytest -s`): the 45 tests of this file take 4.7 s;
9 084 launches, all 9 084 returned the reference, and 6 041 refusals, each with the text expected_refusal predicted (the sweep of (a)
makes 14 014 of the attempts: 53 ids x 13 cases x 4 forms x 3 placements / 4 split counts).  The largest value assert_exact's bound sees
in (a) is 9 679 (stem) against the limit of 4 194 304 (2^24 steps of 1/4); 734 091 in the uint8 stems, 1.7e6 in the split-bf16 test.
"""
import dataclasses
import re

import numpy as np
import pytest
import torch

import _conv3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = -12345.0
GUARD = 1024  # floats of NaN / sentinel on either side of every operand, inside its allocation

RAN = set()        # (id, family, case, form, placement, splits > 1) of every launch that returned the reference
REFUSED = set()    # (family, the documented text)
CASES_RUN = set()  # the cases of (a) that ran in this session
PROBED = set()     # (id, case) the gather probe returned the reference on
BF16 = set()       # (id, case, splits, which operand carries the lo image)
FUSED = set()      # (entry point, form) of (d)
COUNT = {"launches": 0, "references": 0, "refusals": 0}

# (residual, ReLU, out is the residual buffer)
FORMS = {"relu": (False, True, False), "res_relu": (True, True, False), "res": (True, False, False), "res_relu_inplace": (True, True, True)}
PLACEMENTS = ("dense", "slices", "off1")
PLAIN_FAMILIES = ("generic", "fast", "dma3", "dma4", "bf16x3", "dma2")  # every family outside TSPAN, MIXED, PERSIST and the T-fold
IDS = [c[0] for c in R.CASES]


def _mods():
    from anomaly_detection_on_video_amd import _lib, ops

    return _lib, ops


_ALGOS = {}


def _algos():
    if not _ALGOS:
        _ALGOS.update(R.algos())
    return _ALGOS


def _bits(t):
    return t.view(torch.int32)


class Guarded:
    """A tensor on the device inside a larger `fill`-filled allocation: `view` (dense, or a channel slice [lo, lo + c) of a wider NCDHW
    tensor that is itself `fill`), the allocation as it was handed over, and the flat indices of everything but the view"""

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

    def changed(self, base=None):
        """0-dim bool tensor: some bit of the allocation differs from what was handed over"""
        return (_bits(self.base if base is None else base) != _bits(self.pristine)).any()

    def outside_changed(self, base):
        return (_bits(base).index_select(0, self.outside) != _bits(self.pristine).index_select(0, self.outside)).any()


def _wrong_elements(got, want, limit=4):
    """'n wrong elements: (b, c, t, h, w) got / want, ...'"""
    got, want = got.detach().cpu(), want.detach().cpu()
    bad = (got != want).reshape(-1).nonzero().reshape(-1)
    first = []
    for i in bad[:limit].tolist():
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
        first.append(f"{idx} got {float(got.reshape(-1)[i])!r} want {float(want.reshape(-1)[i])!r}")
    return f"{bad.numel()} wrong elements of {got.numel()}: " + "; ".join(first)


# ---- (a) every id, form, placement and split count ---------------------------------------------------------------------------------------
class Problem:
    """One geometry case: integer operands, the exact BatchNorm, the fp64 reference of every form (computed once), the packed conv"""

    def __init__(self, case):
        _lib, ops = _mods()
        self.case = case
        self.name, self.cin, self.cout, self.k, self.s, self.p, self.bthw = case
        self.x, self.w, self.res = R.operands(case)
        (gamma, beta, mean, var), (self.scale, self.shift) = R.exact_bn(self.name, self.cout)
        self.top = R.assert_exact(self.x, self.w, self.scale, self.shift, self.res, self.s, self.p)
        acc = R.conv_ref(self.x, self.w, self.s, self.p)
        self.ref = {}
        for form, (residual, relu, _inplace) in FORMS.items():
            y = R.bn_act_ref(acc, self.scale, self.shift, self.res if residual else None, relu)
            assert torch.equal(y.float().double(), y)
            self.ref[form] = y.float().to(DEV)
        self.pc = ops.pack_conv(self.w.to(DEV), gamma.to(DEV), beta.to(DEV), mean.to(DEV), var.to(DEV), 0.0, self.s, self.p, name=f"edges.{self.name}")
        # advhip_bn_fold_f32: scale = gamma / sqrt(var + eps), shift = beta - mean * scale, exact on these values
        assert torch.equal(self.pc.scale.cpu(), self.scale) and torch.equal(self.pc.shift.cpu(), self.shift), "advhip_bn_fold_f32 differs from the exact fold"
        # on the non-dense placements the packed weights sit between NaN, 16-byte aligned (the gather tables are not poisoned: a
        # poisoned offset could send a correct kernel out of its allocation)
        self.w_guarded = Guarded(self.pc.w_packed.cpu(), NAN)
        assert self.w_guarded.view.data_ptr() % 16 == 0 and self.w_guarded.view.is_contiguous()
        self.pc_rehomed = dataclasses.replace(self.pc, w_packed=self.w_guarded.view)
        self.place = {}

    def placement(self, which):
        """-> (x, residual, out) as Guarded: dense and 16-byte aligned; channel slices of wider tensors; the same with x's base one float on"""
        if which not in self.place:
            sent = torch.full(tuple(self.res.shape), SENT)
            if which == "dense":
                g = (Guarded(self.x, NAN), Guarded(self.res, NAN), Guarded(sent, SENT))
                assert g[0].view.is_contiguous() and g[0].view.data_ptr() % 16 == 0
            else:
                g = (Guarded(self.x, NAN, offset=0 if which == "slices" else 1, wide=8, lo=4), Guarded(self.res, NAN), Guarded(sent, SENT, wide=8, lo=4))
                assert g[0].view.data_ptr() % 16 == (0 if which == "slices" else 4)
                assert self.bthw[0] == 1 or not (g[0].view.is_contiguous() or g[2].view.is_contiguous())
            assert g[1].view.is_contiguous() and g[1].view.data_ptr() % 16 == 0 and g[2].view.data_ptr() % 16 == 0
            self.place[which] = g
        return self.place[which]


_PROBLEMS = {}


def _problem(case):
    if case[0] not in _PROBLEMS:
        _PROBLEMS[case[0]] = Problem(case)
    return _PROBLEMS[case[0]]


def _sweep(prob, forms=tuple(FORMS), placements=PLACEMENTS, ids=None):
    """Every id x form x placement x split count of one case -> the list of complaints.  One synchronisation for the whole case."""
    _lib, ops = _mods()
    bad, pend = [], []
    for algo, info in _algos().items():
        if ids is not None and algo not in ids:
            continue
        fam = info[0]
        top = R.max_splits(info, prob.case)
        for form in forms:
            residual, relu, inplace = FORMS[form]
            for where in (placements if residual else ("dense",)):
                xg, rg, og = prob.placement(where)
                x = xg.view
                x16 = x.data_ptr() % 16 == 0 and ops.batch_stride(x) % 4 == 0
                pc = prob.pc if where == "dense" else prob.pc_rehomed
                for splits in (sorted({1, 2, 3, top}) if where == "dense" else (1,)):
                    what = f"{prob.name} id {algo} ({fam} {info[1]}x{info[2]}x{info[3]}) form {form} placement {where} splits {splits}"
                    want = R.expected_refusal(info, prob.case, FORMS[form], splits, x16)
                    if inplace:  # out is the residual buffer: a dense view between NaN
                        out, out_base = rg.fresh()
                        res_t, guard = out, rg
                    else:
                        out, out_base = og.fresh()
                        res_t, guard = (rg.view if residual else None), og
                    try:
                        got = ops.conv3d_bn_act(x, pc, relu=relu, residual=res_t, algo=algo, out=out, splits=splits)
                    except _lib.HipExtensionError as e:
                        COUNT["refusals"] += 1
                        if want is None or not re.search(want, str(e)):
                            bad.append(f"{what}: refused with '{e}', expected {'a result' if want is None else repr(want)}")
                        else:
                            REFUSED.add((fam, want))
                        continue
                    COUNT["launches"] += 1
                    if want is not None:
                        bad.append(f"{what}: ran, although the launcher documents '{want}'")
                        continue
                    assert got.data_ptr() == out.data_ptr()
                    flags = [(out != prob.ref[form]).any(), guard.outside_changed(out_base), xg.changed()]
                    flags.append(rg.changed() if residual and not inplace else flags[2])
                    flags.append(prob.w_guarded.changed() if where != "dense" else flags[2])
                    pend.append((what, (algo, fam, prob.name, form, where, splits > 1), form, out, torch.stack(flags)))
    flags = torch.stack([p[4] for p in pend]).cpu().tolist() if pend else []
    for (wrong, sentinel, xbad, rbad, wbad), (what, key, form, out, _f) in zip(flags, pend):
        if wrong:
            bad.append(f"{what}: " + _wrong_elements(out, prob.ref[form]))
        if sentinel:
            bad.append(f"{what}: the surroundings of the output changed")
        if xbad or rbad or wbad:
            bad.append(f"{what}: an operand or its surroundings changed (x {xbad}, residual {rbad}, weights {wbad})")
        if not (wrong or sentinel or xbad or rbad or wbad):
            RAN.add(key)
            COUNT["references"] += 1
    return bad


def _report(bad):
    assert not bad, f"{len(bad)} complaints, the first 20:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_id_returns_the_reference_or_its_documented_refusal(case):
    """Every accepted id x (no residual, ReLU), (residual, ReLU), (residual, none), (residual, ReLU, in place) x dense / channel slices /
    x off by one float x splits 1, 2, 3 and the largest the id accepts (dense only): the documented refusal, or the fp64 reference element
    by element, with the sentinel, the NaN around the operands and the operands themselves untouched."""
    prob = _problem(case)
    print(f"{prob.name}: largest value the bound of assert_exact sees {prob.top:.0f} of {R.EXACT_LIMIT:.0f}")
    bad = _sweep(prob)
    CASES_RUN.add(prob.name)
    _report(bad)


# ---- (b) the gather probe --------------------------------------------------------------------------------------------------------------------
def _decode(v, shape):
    """an output value of the probe back to the input element it names"""
    if v == 0.0:
        return "0 (a tap in the padding)"
    if v != v or v != int(v) or not 1 <= v <= int(np.prod(shape)):
        return f"{v!r} (no element's id)"
    return f"x{tuple(int(i) for i in np.unravel_index(int(v) - 1, shape))}"


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_gather_probe_names_the_element_every_tap_reads(case):
    """One-hot weights -- output channel c of set s carries a single 1 at flattened tap ((s Cout + c) 11) mod K -- on x = its own flat
    index + 1, scale 1, shift 0, no activation: every output is the id of the one input element it must have read, or 0 where the tap lies
    in the padding.  Every id that runs the case unsplit; sets until every (ci, dt, dh, dw) has been probed, 8 at the most (stem: 512 of
    its 735 taps)."""
    _lib, ops = _mods()
    name, cin, cout, k, s, p, (b, t, h, w) = case
    xshape = (b, cin, t, h, w)
    px = R.probe_x(xshape)
    xg = Guarded(px, NAN)
    one, zero = torch.ones(cout), torch.zeros(cout)
    K = cin * k[0] * k[1] * k[2]
    bad, pend = [], []
    for si in range(R.probe_sets(cout, cin, k)):
        pw = R.probe_weights(cout, cin, k, si)
        R.assert_exact(px, pw, one, zero, None, s, p)
        ref = R.conv_ref(px, pw, s, p).float().to(DEV)
        pc = ops.pack_conv(pw.to(DEV), one.to(DEV), zero.to(DEV), zero.to(DEV), one.to(DEV), 0.0, s, p, name=f"probe.{name}.{si}")
        assert torch.equal(pc.scale.cpu(), one) and torch.equal(pc.shift.cpu(), zero)
        for algo, info in _algos().items():
            if R.expected_refusal(info, case, (False, False, False), 1, True) is not None:
                continue
            out = ops.conv3d_bn_act(xg.view, pc, relu=False, algo=algo, splits=1)
            COUNT["launches"] += 1
            pend.append((algo, info, si, out, ref, (out != ref).any()))
    flags = torch.stack([q[5] for q in pend]).cpu().tolist()
    for wrong, (algo, info, si, out, ref, _f) in zip(flags, pend):
        if not wrong:
            PROBED.add((algo, name))
            COUNT["references"] += 1
            continue
        got, want = out.cpu(), ref.cpu()
        idx = (got != want).nonzero()
        lines = []
        for ob, oc, ot, oh, ow in idx[:4].tolist():
            tap = R.probe_tap(oc, si, cout, K)
            ci, dt, dh, dw = (int(v) for v in np.unravel_index(tap, (cin,) + tuple(k)))
            lines.append(f"y{(ob, oc, ot, oh, ow)} = tap (ci {ci}, dt {dt}, dh {dh}, dw {dw}) read {_decode(float(got[ob, oc, ot, oh, ow]), xshape)}, "
                         f"must read {_decode(float(want[ob, oc, ot, oh, ow]), xshape)}")
        bad.append(f"{name} id {algo} {info} weight set {si}: {idx.shape[0]} wrong outputs: " + "; ".join(lines))
    assert pend and bool(xg.changed()) is False
    _report(bad)


# ---- (c) the split-bf16 kernels: the lo image of either operand, exactly ---------------------------------------------------------------------
def test_split_bf16_is_exact_when_one_operand_fits_the_hi_image():
    """x = 256 a + b with a, b in -3..3 has 16 significant bits at the most: hi + lo is exact under round-to-nearest.  With w in -3..3 (its
    lo image is 0) hi*hi + hi*lo + lo*hi is the exact product, so the BF16X3 ids must return the reference (largest sum: 1.7e6 on the stem,
    below 2^24); then the two swapped: the lo path of either operand."""
    _lib, ops = _mods()
    bad, pend = [], []
    for name in ("w33.s1", "stem", "t3", "k1.98"):
        case = R.CASE[name]
        _, cin, cout, k, s, p, (b, t, h, w) = case
        one, zero = torch.ones(cout), torch.zeros(cout)
        xs, ws, _ = R.operands(case, "bf.")
        for lo_in, x, wt in (("x", R.hi_image_pair(f"bf.{name}.x", tuple(xs.shape)), ws), ("w", xs, R.hi_image_pair(f"bf.{name}.w", tuple(ws.shape)))):
            R.assert_exact(x, wt, one, zero, None, s, p)
            ref = R.conv_ref(x, wt, s, p).float().to(DEV)
            xg = Guarded(x, NAN)
            pc = ops.pack_conv(wt.to(DEV), one.to(DEV), zero.to(DEV), zero.to(DEV), one.to(DEV), 0.0, s, p, name=f"bf16.{name}.{lo_in}")
            for algo, info in _algos().items():
                if info[0] != "bf16x3":
                    continue
                for splits in (1, 2):
                    what = f"{name} id {algo} {info} lo image of {lo_in} splits {splits}"
                    want = R.expected_refusal(info, case, (False, False, False), splits, True)
                    try:
                        out = ops.conv3d_bn_act(xg.view, pc, relu=False, algo=algo, splits=splits)
                    except _lib.HipExtensionError as e:
                        COUNT["refusals"] += 1
                        if want is None or not re.search(want, str(e)):
                            bad.append(f"{what}: refused with '{e}', expected {'a result' if want is None else repr(want)}")
                        else:
                            REFUSED.add((info[0], want))
                        continue
                    COUNT["launches"] += 1
                    if want is not None:
                        bad.append(f"{what}: ran, although the launcher documents '{want}'")
                        continue
                    pend.append((what, (algo, name, splits, lo_in), out, ref, (out != ref).any() | xg.changed()))
    flags = torch.stack([q[4] for q in pend]).cpu().tolist()
    for wrong, (what, key, out, ref, _f) in zip(flags, pend):
        if wrong:
            bad.append(f"{what}: " + _wrong_elements(out, ref))
        else:
            BF16.add(key)
            COUNT["references"] += 1
    _report(bad)
    assert {(k_[1], k_[2], k_[3]) for k_ in BF16} == {(n, sp, lo) for n in ("w33.s1", "stem", "t3", "k1.98") for sp in (1, 2) for lo in ("x", "w")}


# ---- (d) the fused launches against the fp64 conv + pool ---------------------------------------------------------------------------------------
def _fused_operands(tag, cin, cout, k, s, p, bthw, x=None):
    """-> x, w, (scale, shift), the packed conv, the fp64 conv accumulator"""
    _lib, ops = _mods()
    x = R.ints(f"fused.{tag}.x", (bthw[0], cin) + tuple(bthw[1:])) if x is None else x
    wt = R.ints(f"fused.{tag}.w", (cout, cin) + tuple(k))
    (gamma, beta, mean, var), (scale, shift) = R.exact_bn(f"fused.{tag}", cout)
    pc = ops.pack_conv(wt.to(DEV), gamma.to(DEV), beta.to(DEV), mean.to(DEV), var.to(DEV), 0.0, s, p, name=f"fused.{tag}")
    assert torch.equal(pc.scale.cpu(), scale) and torch.equal(pc.shift.cpu(), shift)
    return x, wt, (scale, shift), pc, R.conv_ref(x, wt, s, p)


def _check_out(what, og, out, out_base, ref, bad):
    if bool((out != ref).any()):
        bad.append(f"{what}: " + _wrong_elements(out, ref))
    elif bool(og.outside_changed(out_base)):
        bad.append(f"{what}: the surroundings of the output changed")
    else:
        COUNT["references"] += 1
        return True
    return False


STEM = (3, 64, (5, 7, 7), (2, 2, 2), (2, 3, 3))
POOL233_CASES = [("stem",) + STEM + ((2, 5, 11, 16),), ("stem",) + STEM + ((1, 4, 38, 40),), ("stem",) + STEM + ((1, 8, 22, 24),),
                 ("s133", 16, 128, (1, 3, 3), (1, 1, 2), (0, 1, 1), (1, 4, 21, 64))]


@pytest.mark.parametrize("case", POOL233_CASES, ids=[f"{c[0]}-{c[6]}" for c in POOL233_CASES])
def test_conv_maxpool233_every_form_equals_the_reference(case):
    """ops.conv3d_bn_relu_maxpool233: the 4-byte gather, the column-parity planes, the planes with the launch split by pool window in t --
    (2,5,11,16): the smallest width the planes admit; (1,4,38,40): bricks outside the tensor; (1,8,22,24): interior and border pool
    windows in t; s133: kw = 3, stride 2 along w only, two n-tiles."""
    _lib, ops = _mods()
    name, cin, cout, k, s, p, bthw = case
    x, wt, (scale, shift), pc, acc = _fused_operands(f"p233.{name}.{bthw}", cin, cout, k, s, p, bthw)
    R.assert_exact(x, wt, scale, shift, None, s, p)
    ref64 = R.maxpool233_ref(R.bn_act_ref(acc, scale, shift, None, True))
    ref = ref64.float().to(DEV)
    assert ops.s2w_ok(pc, bthw[3])
    xg = Guarded(x, NAN)
    og = Guarded(torch.full(tuple(ref.shape), SENT), SENT, wide=8, lo=4)
    bad = []
    for form, kw in (("plain", dict(s2w=False)), ("planes", dict(s2w=True, border=False)), ("planes+border", dict(s2w=True, border=True))):
        out, out_base = og.fresh()
        got = ops.conv3d_bn_relu_maxpool233(xg.view, pc, out=out, **kw)
        COUNT["launches"] += 1
        assert got.data_ptr() == out.data_ptr()
        if _check_out(f"pool233 {name} {bthw} {form}", og, out, out_base, ref, bad):
            FUSED.add(("pool233", form))
    assert not bool(xg.changed())
    _report(bad)


@pytest.mark.parametrize("bthw", [(1, 2, 7, 9), (3, 5, 13, 11), (1, 6, 1, 1)], ids=str)
@pytest.mark.parametrize("chans", [(64, 256), (128, 64)], ids=lambda c: f"{c[0]}to{c[1]}")
def test_conv_maxpool211_equals_the_reference(chans, bthw):
    """ops.conv3d_bn_act_maxpool211 on x as a channel slice of a NaN-filled buffer, the three residual / ReLU forms; T = 5: the last
    frame belongs to no pooling pair."""
    _lib, ops = _mods()
    cin, cout = chans
    one = (1, 1, 1)
    x, wt, (scale, shift), pc, acc = _fused_operands(f"p211.{chans}.{bthw}", cin, cout, one, one, (0, 0, 0), bthw)
    res = R.ints(f"fused.p211.{chans}.{bthw}.r", tuple(acc.shape))
    R.assert_exact(x, wt, scale, shift, res, one, (0, 0, 0))
    xg, rg = Guarded(x, NAN, wide=8, lo=4), Guarded(res, NAN)
    bad = []
    for form in ("relu", "res_relu", "res"):
        residual, relu, _ = FORMS[form]
        ref = R.maxpool211_ref(R.bn_act_ref(acc, scale, shift, res if residual else None, relu)).float().to(DEV)
        og = Guarded(torch.full(tuple(ref.shape), SENT), SENT, wide=8, lo=4)
        out, out_base = og.fresh()
        ops.conv3d_bn_act_maxpool211(xg.view, pc, relu=relu, residual=rg.view if residual else None, out=out)
        COUNT["launches"] += 1
        if _check_out(f"pool211 {chans} {bthw} {form}", og, out, out_base, ref, bad):
            FUSED.add(("pool211", form))
    assert not bool(xg.changed()) and not bool(rg.changed())
    _report(bad)


@pytest.mark.parametrize("shape", [(3, 64, 128, (2, 7, 7)), (2, 96, 64, (1, 8, 8)), (4, 32, 64, (1, 2, 2))], ids=str)
def test_conv_mean_equals_the_rounded_quotient(shape):
    """ops.conv3d_bn_act_avgpool on 98, 64 and 4 positions: the sum is exact and the kernel ends in one correctly rounded fp32 division, so
    the result is float32(sum / n)."""
    _lib, ops = _mods()
    b, cin, cout, thw = shape
    one = (1, 1, 1)
    x, wt, (scale, shift), pc, acc = _fused_operands(f"mean.{shape}", cin, cout, one, one, (0, 0, 0), (b,) + thw)
    res = R.ints(f"fused.mean.{shape}.r", tuple(acc.shape))
    top = R.assert_exact(x, wt, scale, shift, res, one, (0, 0, 0))
    n = thw[0] * thw[1] * thw[2]
    assert top * n < R.EXACT_LIMIT  # the sum over the positions is exact too
    xg, rg = Guarded(x, NAN), Guarded(res, NAN)
    bad = []
    for form in ("relu", "res_relu", "res"):
        residual, relu, _ = FORMS[form]
        y = R.bn_act_ref(acc, scale, shift, res if residual else None, relu)
        total = y.sum(dim=(2, 3, 4), keepdim=True)
        assert torch.equal(total.float().double(), total)
        ref = (total / n).float().to(DEV)  # (fp64 -> fp32 of a quotient of two fp32 values: the correctly rounded fp32 quotient)
        out = ops.conv3d_bn_act_avgpool(xg.view, pc, relu=relu, residual=rg.view if residual else None)
        COUNT["launches"] += 1
        if bool((out != ref).any()):
            bad.append(f"conv + mean {shape} {form}: " + _wrong_elements(out, ref))
        else:
            FUSED.add(("mean", form))
            COUNT["references"] += 1
    assert not bool(xg.changed()) and not bool(rg.changed())
    _report(bad)


U8_CASES = [((16, 40, 52, 3), 8, 32, ("taps", "bytes", "planes", "planes+border")), ((10, 33, 61, 3), 5, 23, ("taps", "bytes"))]
_U8_REFS = {}


def _u8_reference(fshape, fpc, crop):
    """frames, the packed stem, the fp64 reference rows of every crop-clip of the video -- computed once"""
    key = (fshape, fpc, crop)
    if key not in _U8_REFS:
        from oracle import host_oracle

        frames = R.ints(f"fused.u8.{fshape}", fshape, 0, 255)
        crops = host_oracle.ten_crop_clips(frames.numpy().astype(np.uint8), fpc, crop, 114.0, 64.0)  # (clips, 10, C, T, crop, crop)
        xn = torch.from_numpy(crops).reshape((-1,) + crops.shape[2:])
        assert torch.equal(xn * 64.0, (xn * 64.0).round())  # (pixel - 114) / 64: exact
        cin, cout, k, s, p = STEM
        _, wt, (scale, shift), pc, acc = _fused_operands(f"u8.{fshape}", cin, cout, k, s, p, None, x=xn)
        # every value any of the stems can form -- sums of w * pixel (integers), the per-border-class correction -114 * sum w, the
        # products with scale / 64 (a power of two) -- is a multiple of 1/256 whose size the bound on the raw pixels covers
        R.assert_exact(xn * 64.0 + 114.0, wt, scale, shift, None, s, p)
        ref = R.maxpool233_ref(R.bn_act_ref(acc, scale, shift, None, True))
        assert torch.equal(ref.float().double(), ref)
        _U8_REFS[key] = (frames.to(torch.uint8), pc, ref.float().to(DEV))
    return _U8_REFS[key]


@pytest.mark.parametrize("surround", [0, 255])
@pytest.mark.parametrize("case", U8_CASES, ids=[str(c[0]) for c in U8_CASES])
def test_u8_stems_equal_the_reference_on_numpy_tencrop(case, surround, monkeypatch):
    """ops.conv3d_u8_tencrop_bn_relu_maxpool233 under U8_STEM_FORM "taps" and "bytes", and ops.tencrop_planes_u8 + the planes-form stem:
    mean 114 and std 64 make (pixel - mean) / std, the border corrections and scale / std exact.  The crops of the reference are the
    numpy TenCrop of oracle/host_oracle on the raw bytes.  The frames sit in a larger uint8 buffer filled with `surround`."""
    _lib, ops = _mods()
    fshape, fpc, crop, forms = case
    frames, pc, ref = _u8_reference(fshape, fpc, crop)
    n = ref.shape[0]
    buf = torch.full((frames.numel() + 2 * 4096,), surround, dtype=torch.uint8)
    buf[4096 : 4096 + frames.numel()] = frames.reshape(-1)
    buf = buf.to(DEV)
    pristine = buf.clone()
    fd = buf[4096 : 4096 + frames.numel()].view(fshape)
    bad = []
    for form in forms:
        for first, count in ((0, n), (7, 9)):  # all of them, and a range that starts inside the first clip and ends inside the second
            want = ref[first : first + count]
            og = Guarded(torch.full(tuple(want.shape), SENT), SENT, wide=8, lo=4)
            out, out_base = og.fresh()
            if form in ("taps", "bytes"):
                monkeypatch.setattr(ops, "U8_STEM_FORM", form)
                ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, first, count, frames_per_clip=fpc, crop=crop, out=out, mean=114.0, std=64.0)
            else:
                xs = ops.tencrop_planes_u8(fd, first, count, frames_per_clip=fpc, crop=crop, mean=114.0, std=64.0)
                ops.conv3d_s2w_bn_relu_maxpool233(xs, pc, out=out, border=form == "planes+border")
            COUNT["launches"] += 1
            if _check_out(f"u8 stem {fshape} {form} crop-clips [{first}, {first + count}) surroundings {surround}", og, out, out_base, want, bad):
                FUSED.add(("u8", form))
    assert torch.equal(buf, pristine)
    _report(bad)


# ---- (e) what all of the above covered -----------------------------------------------------------------------------------------------------------
def _tuned_families():
    """the families of the ids the tuned tables select"""
    import glob
    import json
    import os

    from anomaly_detection_on_video_amd import tuned

    fams = set()
    for path in glob.glob(os.path.join(os.path.dirname(tuned.__file__), "tuned", "gfx950*.json")):
        for algo, _splits in json.load(open(path)).values():
            fams.add(_algos()[algo][0])
    return fams


def test_every_family_met_every_edge():
    """What the tests above recorded.  Every accepted id returned the reference on some case; every id outside TSPAN, MIXED, PERSIST and
    the T-fold on a padded spatial window, on a strided conv, on k1.98 and with splits > 1; TSPAN on t3; every T-fold id on t3.T2 and t3.T1;
    MIXED and PERSIST on k1.260; every family the tuned tables select on both non-dense placements; every refusal was predicted."""
    if not CASES_RUN:  # selected on its own: one parameter set of each of the others
        test_every_id_returns_the_reference_or_its_documented_refusal(R.CASE["k1.98"])
        test_gather_probe_names_the_element_every_tap_reads(R.CASE["k333.small"])
        test_split_bf16_is_exact_when_one_operand_fits_the_hi_image()
        test_conv_maxpool233_every_form_equals_the_reference(POOL233_CASES[0])
        test_conv_maxpool211_equals_the_reference((128, 64), (1, 2, 7, 9))
        test_conv_mean_equals_the_rounded_quotient((4, 32, 64, (1, 2, 2)))
    algos = _algos()
    print("launches / references returned / refusals:", COUNT)
    print("refusals seen (family, text):", sorted(REFUSED))

    def ran(algo, case, **kw):
        """some launch of `algo` on `case` returned the reference (with the given form / placement / split?)"""
        return any(a == algo and c == case and all({"form": f, "where": w, "split": sp}[k_] == v for k_, v in kw.items())
                   for a, _fam, c, f, w, sp in RAN)

    missing = []

    def need(cond, what):
        if not cond:
            missing.append(what)

    whole = CASES_RUN == set(IDS)
    if whole:
        for algo in algos:
            need(any(a == algo for a, *_ in RAN), f"id {algo} returned the reference on no case")
    for algo, info in algos.items():
        fam = info[0]
        if fam in PLAIN_FAMILIES:
            for c in ("w33.s1", "w33.s2", "stem", "odd333", "k333.small"):  # a padded spatial window (Cout = 64 but for w33.s2)
                if c in CASES_RUN and (info[2] <= 64 or c == "w33.s2"):
                    need(ran(algo, c), f"id {algo} ({fam}) on the padded window {c}")
            for c in ("w33.s2", "k1.s2"):  # a strided conv (Cout = 128: every N tile divides it)
                if c in CASES_RUN:
                    need(ran(algo, c), f"id {algo} ({fam}) on the strided conv {c}")
            if "k1.98" in CASES_RUN:
                need(ran(algo, "k1.98"), f"id {algo} ({fam}) on k1.98")
                need(ran(algo, "k1.98", split=True), f"id {algo} ({fam}) with splits > 1")
        if fam == "tspan" and "t3" in CASES_RUN:
            need(ran(algo, "t3"), "TSPAN on t3")
        if fam == "tfold":
            if "t3.T2" in CASES_RUN:
                need(ran(algo, "t3.T2"), f"T-fold id {algo} on t3.T2")
            if "t3.T1" in CASES_RUN and info[2] <= 64:  # (Cout * T = 64 there: the 128-wide N tiles refuse it, as documented)
                need(ran(algo, "t3.T1"), f"T-fold id {algo} on t3.T1")
        if fam in ("mixed", "persist") and "k1.260" in CASES_RUN:
            need(ran(algo, "k1.260"), f"id {algo} ({fam}) on k1.260")
    if whole:
        tuned_fams = _tuned_families()
        assert tuned_fams <= {"dma3", "dma4", "dma2", "tspan", "tfold", "bf16x3"}, tuned_fams
        for fam in tuned_fams:
            for where in ("slices", "off1"):
                need(any(f == fam and w == where for _a, f, _c, _form, w, _sp in RAN), f"family {fam} on placement {where}")
        for lo in ("x", "w"):
            need({a for a, _n, _sp, l_ in BF16 if l_ == lo} == {a for a, i in algos.items() if i[0] == "bf16x3"}, f"every BF16X3 id with the lo image of {lo}")
        need(FUSED >= {("pool233", f) for f in ("plain", "planes", "planes+border")} | {("pool211", f) for f in ("relu", "res_relu", "res")}
             | {("mean", f) for f in ("relu", "res_relu", "res")} | {("u8", f) for f in ("taps", "bytes", "planes", "planes+border")}, f"fused forms: {sorted(FUSED)}")
        need({a for a, _c in PROBED} >= {a for a, i in algos.items() if i[0] in PLAIN_FAMILIES}, "the gather probe on every plain id")
    # every refusal seen is one expected_refusal predicted (the sweeps complain about any other); every family is among them or ran
    assert all(isinstance(t, str) and t for _f, t in REFUSED)
    assert not missing, "\n".join(missing)
