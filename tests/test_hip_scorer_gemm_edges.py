"""The scorer's GEMM-shaped kernels at their tile edges: exact, element by element, with poisoned surroundings.

  mgfn_ops.conv_cn (advhip_conv3d_bn_act_ex_f32 on a (C, B, T) activation, k = 1 / 3) on EVERY algorithm id the library accepts, with
      the tile and the K slices pinned (conv_cn's `algo` / `splits`); pack_kc / pack_dx; the in-launch split-K and its counters
  ops.gemm_nt / gemm_nt_group / advhip_sum_slabs_f32 and the C entry points behind them (pitches, bases, ldc, slab strides, refusals)
  ops.bgemm (four operand layouts, both tile heights, vector loads on and off) and ops.softmax_rows

Integer-valued operands (tests/_gemm_ref.py) make every fp32 result exact for any summation order, so results must EQUAL the fp64
reference; operands in eighths make the pre-activation exact, so GELU / GELU' are compared at a known z, per element, against a
bound measured on the host (4 x the worst error of torch's own fp32 evaluation, in units of 2^-24 max(1, |z|) for GELU and 2^-24
for GELU' and exp).  Operands are views into NaN-filled buffers, outputs (where the entry point takes one) views into
sentinel-filled ones.  For every (id, epilogue form) there are two outcomes: the refusal the launcher documents, or the reference.

Worst figures seen on an MI355X, in those units (device / host / allowed = 4 x host):
  conv GELU   (codes 2 and 3: y)        1.46 / 4.14 / 16.5   the 128 x 128 tiles' pipelined forms and the generic epilogue alike
  conv GELU'  (code 3: second output)   2.07 / 2.95 / 11.8
  code 3 against code 2 + GELU'(z)      y: 0 (the same bits on every id), second output: 2.0 (one ulp; the one-erf form)
  conv x GELU'(dact_z)                  0.17 of its bound
  bgemm GELU  (act 2)                   1.46 / 4.14 / 16.5
  softmax, relative                     2.2 (n = 2) ... 3.7 (n = 129), 7.7 (n = 16 384) against 18.4 ... 20.4, 273.4; host exp 0.86
(printed by the tests on every run: `pytest -s`).

test_every_form_ran_on_both_branches_or_was_refused_as_documented reads what the tests above it recorded (selected on its own, it runs
one parameter set of each of them first).
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _gemm_ref as R
from anomaly_detection_on_video_amd.weights import synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = -12345.0
U24 = R.U24

RAN = set()      # (family, form, n % 4 == 0) of every launch that returned the reference
EPI = set()      # (epilogue body, n % 4 == 0) of the same launches, by the dispatch rule of igemm_epilogue
REFUSED = set()  # (family, form, the documented text)
SEEN = set()     # (family, form) of every attempt

# epilogue forms of conv_cn: which operands a call carries
FORMS = {
    "shift": dict(),
    "res": dict(residual=True),
    "relu": dict(act=R.ACT_RELU),
    "mul": dict(act=R.ACT_MUL, dact=True),
    "preact": dict(preact=True),
    "ln": dict(ln=True),
    "ln_res": dict(ln=True, residual=True),
    "gelu": dict(act=R.ACT_GELU, preact=True),
    "gelu_d": dict(act=R.ACT_GELU_D, preact=True),
    "dact": dict(dact=True),
}
INT_FORMS = ("shift", "res", "relu", "mul", "preact", "ln", "ln_res")
GELU_FORMS = ("gelu", "gelu_d", "dact")


def _mods():
    from anomaly_detection_on_video_amd import _lib, mgfn_ops, ops

    return _lib, mgfn_ops, ops


_ALGOS = {}


def _algos():
    """{id: (family, BM, BN, BK)} from advhip_conv3d_algo_info; a T-fold id's family is 'tfold' here (the query reports the kernel it runs)"""
    if not _ALGOS:
        from test_conv_algo_table import _accepted

        _lib = _mods()[0]
        for a, info in sorted(_accepted().items()):
            _ALGOS[a] = (("tfold",) + tuple(info[1:])) if _lib.is_tfold(a) else tuple(info)
    return _ALGOS


_REDUCES = {}


def _reduces_in_launch(algo):
    """Whether `algo` sums its K slices inside the launch, read off the size of the workspace it asks for: [splits][M * Cout] slabs for a
    second launch, or one arrival counter per tile (padded to 256 bytes) + [tiles][splits][BM * BN] partial tiles (conv_igemm.hip: SplitLayout)"""
    if algo not in _REDUCES:
        _lib, mgfn_ops, _ = _mods()
        _fam, bm, bn, _bk = _algos()[algo]
        n, cout, s = 260, 128, 2
        got = _lib.load().advhip_conv3d_workspace_bytes(C.byref(mgfn_ops._desc(64, cout, 1, 1, n, 0, algo, s)))
        tiles = -(-n // bm) * (cout // bn)
        slabs, in_launch = s * n * cout * 4, -(-tiles * 4 // 256) * 256 + tiles * s * bm * bn * 4
        assert got in (slabs, in_launch), (algo, got, slabs, in_launch)
        _REDUCES[algo] = got == in_launch
    return _REDUCES[algo]


def _expected_refusal(algo, k, cin, cout, n, form, splits, x16):
    """The text of the precondition (include/advhip.h, the launchers' messages) that this call does not meet, or None: it must run"""
    fam, bm, bn, bk = _algos()[algo]
    f = FORMS[form]
    ln, dact, preact = bool(f.get("ln")), bool(f.get("dact")), bool(f.get("preact"))
    plain = not (ln or dact or preact)  # none of the extra epilogue operands (a residual is not one of them)
    kpad = -(-(cin * k) // 32) * 32
    if fam == "tfold":
        if k != 1:
            return r"ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs a \(kt,1,1\) conv"
        if ln:
            return "ADVHIP_ALGO_TFOLD takes neither the LayerNorm fold"
    if ln and k != 1:
        return "the LayerNorm fold applies to 1x1x1 stride-1 convs"
    if not plain and splits > 1 and not _reduces_in_launch(algo):
        return "need a fused epilogue"
    if cout % bn:
        return f"Cout={cout} not a multiple of the {bn}-wide N tile"
    if splits > -(-kpad // bk):
        return f"bad split count {splits}"
    # rows of 4 positions as 16-byte pieces: an unmasked 1x1x1 conv on aligned rows of a multiple of 4 positions -- or, for the families
    # that pad the rows in the index space (the 2-deep ring and what is built on it), any row length when no extra operand is there
    pads = fam in ("dma2", "tfold", "mixed", "persist")
    a16 = k == 1 and cin * k == kpad and x16 and (n % 4 == 0 or (pads and plain))
    if fam == "tspan":
        return r"ADVHIP_ALGO_TSPAN needs a \(kt,1,1\) stride-1 conv" if k != 1 else "ADVHIP_ALGO_TSPAN runs unsplit on an even number of frames"
    if fam == "mixed" and not (a16 and splits == 1 and plain):
        return "ADVHIP_ALGO_MIXED_128x64 takes unsplit 1x1x1 stride-1 convs on 16-byte aligned rows without the MGFN epilogue operands"
    if fam == "persist":
        if kpad < 64:
            return "the persistent kernels need K >= 64"
        if not (a16 and splits == 1 and not ln and not dact):
            return r"the persistent kernels \(algo \d+\) take unsplit 1x1x1 stride-1 convs on 16-byte aligned rows"
    return None


def _epilogue_body(algo, form, splits):
    """Which epilogue body a launch runs (conv_igemm.hip: igemm_epilogue's dispatch): the pipelined forms for an unsplit launch without
    the LayerNorm fold -- the erf forms on the 128 x 128 tiles only --, the generic body otherwise"""
    _fam, bm, bn, _bk = _algos()[algo]
    f = FORMS[form]
    act, res, dact, y2 = f.get("act", 0), bool(f.get("residual")), bool(f.get("dact")), bool(f.get("preact"))
    if splits != 1:
        return "split-K"
    if not f.get("ln"):
        if bm * bn >= 128 * 128:
            if act == R.ACT_GELU and not res and not dact:
                return "EM_GELU"
            if act == R.ACT_GELU_D and not res and not dact:
                return "EM_GELU2"
            if act <= 1 and not y2 and dact and not res:
                return "EM_DACT"
        if act == R.ACT_MUL and dact and not res and not y2:
            return "EM_MUL"
        if act <= 1 and not y2 and not dact:
            return "EM_RES" if res else "EM_PLAIN"
    return "generic"


class Conv:
    """One conv_cn problem: operands on the device (x inside a NaN-filled buffer), fp64 references per form"""

    def __init__(self, tag, k, cin, cout, b, t, x_offset=0, maker=R.ints, dact=None):
        self.tag, self.k, self.cin, self.cout, self.b, self.t, self.n = tag, k, cin, cout, b, t, b * t
        self.x16 = x_offset % 4 == 0
        self.x, self.w = maker(tag + ".x", (cin, b, t)), maker(tag + ".w", (cout, cin, k))
        self.shift, self.res = maker(tag + ".s", (cout,)), maker(tag + ".r", (cout, b, t))
        self.dact = maker(tag + ".m", (cout, b, t)) if dact is None else dact
        self.ln = (R.ints(tag + ".u", (cout,)), R.ints(tag + ".mu", (self.n,), -2, 2), 2.0 ** R.ints(tag + ".rs", (self.n,), -2, 1))
        self.xd = R.embed(self.x, 64, NAN, x_offset, device=DEV)
        assert self.xd.is_contiguous() and (self.xd.data_ptr() % 16 == 0) == self.x16
        self.wd = self.w.to(DEV)
        self.d = {name: v.to(DEV) for name, v in (("shift", self.shift), ("res", self.res), ("dact", self.dact))}
        self.lnd = tuple(v.to(DEV) for v in self.ln)
        self._packs, self._refs = {}, {}

    def pack(self, algo=None):
        """the weight operand `algo` takes: [K padded to 32][Cout] fp32, or the split-bf16 images of the bf16x3 family"""
        _lib, mgfn_ops, _ = _mods()
        key = algo is not None and _algos()[algo][0] == "bf16x3"
        if key not in self._packs:
            if key:
                d = mgfn_ops._desc(self.cin, self.cout, self.k, 1, 1, 0)
                out = torch.empty((2, self.cout, _lib.load().advhip_conv3d_packed_rows(C.byref(d))), device=DEV, dtype=torch.int16)
                _lib.check(_lib.load().advhip_conv3d_pack_weight_bf16x3(C.byref(d), _lib.ptr(self.wd), _lib.ptr(out), _lib.stream(self.wd)), "pack_weight_bf16x3")
                self._packs[key] = out.view(torch.float32)
            else:
                self._packs[key] = mgfn_ops.pack_kc(self.wd)
        return self._packs[key]

    def call(self, form, algo=None, splits=None):
        _, mgfn_ops, _ = _mods()
        f = FORMS[form]
        return mgfn_ops.conv_cn(self.xd, self.pack(algo), self.cout, self.k, shift=self.d["shift"], residual=self.d["res"] if f.get("residual") else None,
                                act=f.get("act", 0), want_preact=bool(f.get("preact")), dact_z=self.d["dact"] if f.get("dact") else None,
                                ln=self.lnd if f.get("ln") else None, algo=algo, splits=splits)

    def ref64(self, form):
        if form not in self._refs:
            f = FORMS[form]
            self._refs[form] = R.conv_cn_ref(self.x, self.w, self.k, shift=self.shift, residual=self.res if f.get("residual") else None,
                                             act=f.get("act", 0), dact_z=self.dact if f.get("dact") else None,
                                             ln=self.ln if f.get("ln") else None)
        return self._refs[form]

    def ref32(self, form):
        key = form + "/32"
        if key not in self._refs:
            y, z = self.ref64(form)
            assert float(y.abs().max()) < 2 ** 24 and torch.equal(y.float().double(), y) and torch.equal(z.float().double(), z), "not exact in fp32"
            self._refs[key] = (y.float().to(DEV), z.float().to(DEV))
        return self._refs[key]


def _first_diff(got, want):
    i = int((got != want).reshape(-1).float().argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
    return f"first wrong element {idx}: got {float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r}"


def _sweep(case, forms, splits_list=(1,), check=None):
    """Every id x form x split count on one problem: the documented refusal, or `check` (default: the fp64 reference bit for bit, second
    output included).  One synchronisation for the whole problem.  -> the list of complaints"""
    _lib = _mods()[0]
    bad, pend = [], []
    for algo, (fam, bm, bn, bk) in _algos().items():
        for form in forms:
            for s in splits_list:
                what = f"{case.tag} k={case.k} {case.cin}->{case.cout} n={case.b}x{case.t} algo {algo} ({fam} {bm}x{bn}x{bk}) form {form} splits {s}"
                want = _expected_refusal(algo, case.k, case.cin, case.cout, case.n, form, s, case.x16)
                SEEN.add((fam, form))
                try:
                    out = case.call(form, algo, s)
                except _lib.HipExtensionError as e:
                    if want is None or not re.search(want, str(e)):
                        bad.append(f"{what}: refused with '{e}', expected {'a result' if want is None else repr(want)}")
                    else:
                        REFUSED.add((fam, form, want))
                    continue
                if want is not None:
                    bad.append(f"{what}: ran, although the launcher documents '{want}'")
                    continue
                y, z = out if isinstance(out, tuple) else (out, None)
                pend.append((what, algo, fam, form, s, y, z))
    if check is not None:
        return bad + check(pend)
    flags = []
    for what, algo, fam, form, s, y, z in pend:
        ry, rz = case.ref32(form)
        flag = (y != ry).any()  # (a NaN differs from everything)
        flags.append(flag | (z != rz).any() if z is not None else flag)
    flags = torch.stack(flags).cpu().tolist() if flags else []
    for wrong, (what, algo, fam, form, s, y, z) in zip(flags, pend):
        if wrong:
            ry, rz = case.ref32(form)
            bad.append(f"{what}: " + (_first_diff(y, ry) if bool((y != ry).any()) else "second output: " + _first_diff(z, rz)))
        else:
            RAN.add((fam, form, case.n % 4 == 0))
            EPI.add((_epilogue_body(algo, form, s), case.n % 4 == 0))
    return bad


# ---- conv_cn, integers, bit for bit ---------------------------------------------------------------------------------------------------
K1_POSITIONS = (1, 3, 4, 60, 63, 64, 65, 68, 127, 128, 129, 132, 255, 256, 257, 260)
K3_SHAPES = ((1, 1), (3, 1), (2, 2), (5, 3), (3, 4), (5, 13), (2, 32), (3, 33), (2, 64), (1, 65))


@pytest.mark.parametrize("cin", [32, 64, 96])
@pytest.mark.parametrize("cout", [64, 128, 192])
def test_conv_cn_k1_every_id_and_form_equals_the_integers(cin, cout):
    """k = 1: every position count around the 64 / 128 / 256-row tiles on both store widths, K of 2, 4, 6 k-tiles of 16 (an odd number
    of 32-deep ones), x on a 16-byte and on a 4-byte-only aligned base inside NaN.  Codes 0, 1, 4, the residual, the second output
    and the LayerNorm fold (power-of-two rs) equal the fp64 reference on every id, or the id refuses with its documented text."""
    bad = []
    for n in K1_POSITIONS:
        for off in (0, 1) if n in (4, 65, 128, 260) else (0,):
            bad += _sweep(Conv(f"k1.{cin}.{cout}.{n}.{off}", 1, cin, cout, 1, n, off), INT_FORMS)
    assert not bad, f"{len(bad)} complaints, the first 20:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("cout", [64, 128])
def test_conv_cn_k3_taps_are_masked_at_both_ends_of_every_sequence(cin, cout):
    """k = 3, zero padding per sequence: T of 1, 2, 3 (every tap of some position in the padding), m-tiles that straddle sequences,
    Cin * 3 = 96 padded to 128 rows / 192 unpadded; the direct launch on every id, and the unfolded form (_unfold3 + the k = 1 launch on
    3 Cin rows) equal to it."""
    _, mgfn_ops, _ = _mods()
    bad = []
    for b, t in K3_SHAPES:
        case = Conv(f"k3.{cin}.{cout}.{b}.{t}", 3, cin, cout, b, t)
        bad += _sweep(case, ("shift", "res", "relu", "mul", "preact"))
        direct = case.call("res")
        u = mgfn_ops._unfold3(case.xd).view(3 * cin, b, t)
        unfolded = mgfn_ops.conv_cn(u, case.pack(), cout, 1, shift=case.d["shift"], residual=case.d["res"])
        if not (torch.equal(unfolded, direct) and torch.equal(direct, case.ref32("res")[0])):
            bad.append(f"{case.tag}: the unfolded k = 3 form differs from the direct launch / the reference: {_first_diff(unfolded, case.ref32('res')[0])}")
    # the LayerNorm fold is per position of a 1x1x1 conv: a k = 3 launch refuses it (the sweep checks the text)
    bad += _sweep(Conv(f"k3.{cin}.{cout}.ln", 3, cin, cout, 2, 4), ("ln",))
    assert not bad, f"{len(bad)} complaints, the first 20:\n" + "\n".join(bad[:20])


# ---- dX and the packs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t", [(1, 1), (2, 2), (5, 3), (5, 13), (3, 33), (2, 64)])
def test_pack_dx_is_the_exact_adjoint_of_the_forward_conv(b, t):
    _, mgfn_ops, _ = _mods()
    cin, cout = 64, 128
    x, w, dy = R.ints(f"dx.x{b}{t}", (cin, b, t)), R.ints(f"dx.w{b}{t}", (cout, cin, 3)), R.ints(f"dx.g{b}{t}", (cout, b, t))
    xd, wd = R.embed(x, 64, NAN, device=DEV), w.to(DEV)
    dyd = R.embed(dy, 64, NAN, device=DEV)
    dx = mgfn_ops.conv_cn(dyd, mgfn_ops.pack_dx(wd), cin, 3)
    want = R.conv_dx_ref(dy, w, 3).float().to(DEV)
    assert torch.equal(dx, want), _first_diff(dx, want)
    # the residual fold of a block whose skip connection carries dy itself (cout = cin there)
    w2 = R.ints(f"dx.v{b}{t}", (cin, cin, 3))
    dy2 = R.embed(x, 64, NAN, device=DEV)
    dx2 = mgfn_ops.conv_cn(dy2, mgfn_ops.pack_dx(w2.to(DEV)), cin, 3, residual=dy2)
    want2 = (R.conv_dx_ref(x, w2, 3) + x.double()).float().to(DEV)
    assert torch.equal(dx2, want2), _first_diff(dx2, want2)
    # k = 1: the parameter's own [o][c] layout is the operand
    w1 = R.ints(f"dx.u{b}{t}", (cout, cin, 1))
    dx1 = mgfn_ops.conv_cn(dyd, w1.to(DEV).view(cout, cin), cin, 1)
    want1 = R.conv_dx_ref(dy, w1, 1).float().to(DEV)
    assert torch.equal(dx1, want1), _first_diff(dx1, want1)
    # <conv(x), dy> == <x, dx>, as integers, from the kernels' own outputs
    y = mgfn_ops.conv_cn(xd, mgfn_ops.pack_kc(wd), cout, 3)
    lhs, rhs = (y.long() * dyd.long()).sum(), (xd.long() * dx.long()).sum()
    assert int(lhs) == int(rhs) and int(lhs) == int((R.conv_acc(x, w, 3).long() * dy.long()).sum())


@pytest.mark.parametrize("cout,cin,k", [(64, 32, 1), (128, 96, 3), (64, 40, 3), (192, 33, 1), (64, 64, 3), (72, 64, 3), (7, 5, 3)])
def test_packs_against_their_index_formulas(cout, cin, k):
    """pack_kc: [c * k + j][o] = W[o][c][j], rows above Cin * k zero; pack_dx: [o * k + j'][c] = W[o][c][k - 1 - j'], rows above
    Cout * k zero -- on weights whose value names (o, c, j)."""
    _, mgfn_ops, _ = _mods()
    o, c, j = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(k), indexing="ij")
    w = (o * 4096 + c * 4 + j + 1).float()
    assert float(w.max()) < 2 ** 24
    wd = w.to(DEV)
    if cout % 64 == 0:  # (the forward conv's operand exists for Cout % 64 == 0 only)
        got = mgfn_ops.pack_kc(wd).cpu()
        rows = -(-(cin * k) // 32) * 32
        want = torch.zeros((rows, cout))
        want[: cin * k] = w.permute(1, 2, 0).reshape(cin * k, cout)
        assert got.shape == want.shape and torch.equal(got, want)
    got = mgfn_ops.pack_dx(wd).cpu()
    rows = -(-(cout * k) // 32) * 32
    want = torch.zeros((rows, cin))
    want[: cout * k] = w.flip(2).permute(0, 2, 1).reshape(cout * k, cin)
    assert got.shape == want.shape and torch.equal(got, want)


# ---- split-K ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,cin,splits_list,shapes", [(3, 96, (2, 3, 4, 5), ((5, 13), (2, 32), (3, 33))), (1, 64, (2, 4), ((1, 65), (1, 260)))])
def test_conv_cn_split_k_returns_the_same_integers(k, cin, splits_list, shapes):
    """K = 288 (18 / 9 k-tiles) in 2..5 slices and K = 64 in 2 / 4: the ids that reduce in the launch take every form, the others the forms
    without an extra operand (their reduce launch) and refuse the rest; a split count above the k-tiles refuses."""
    bad = []
    for b, t in shapes:
        bad += _sweep(Conv(f"sk.{k}.{cin}.{b}.{t}", k, cin, 128, b, t), INT_FORMS if k == 1 else INT_FORMS[:5], splits_list)
    assert not bad, f"{len(bad)} complaints, the first 20:\n" + "\n".join(bad[:20])
    assert any(_reduces_in_launch(a) for a in _algos()) and not all(_reduces_in_launch(a) for a in _algos())


def test_split_k_counters_are_left_zero_and_carry_no_stale_ticket():
    _, mgfn_ops, ops = _mods()
    dev = torch.device(DEV)
    torch.cuda.synchronize()
    cnt = ops.splitk_counters(dev)
    assert int(cnt.abs().sum()) == 0
    ids = [a for a, info in _algos().items() if _reduces_in_launch(a) and info[0] in ("dma2", "dma3", "dma4") and info[2] == 64 and info[3] == 16]
    assert len(ids) >= 6
    seq = [(3, 96, 5, 13, 2), (1, 64, 1, 260, 4), (3, 96, 3, 33, 5), (1, 64, 1, 65, 2), (3, 96, 2, 32, 3), (1, 64, 1, 260, 2)]
    cases = {s[:4]: Conv("cnt.%d.%d.%d.%d" % s[:4], s[0], s[1], 128, s[2], s[3]) for s in seq}
    flags = []
    for rep in range(2):
        for algo in ids:
            for k, cin, b, t, s in seq:
                case = cases[(k, cin, b, t)]
                for form in ("res", "preact", "mul"):
                    out = case.call(form, algo, s)
                    y = out[0] if isinstance(out, tuple) else out
                    flags.append((y != case.ref32(form)[0]).any())
    assert ops.splitk_counters(dev) is cnt, "a launch of this sequence reported an error (the counter block was dropped)"
    assert not bool(torch.stack(flags).any()) and int(cnt.abs().sum()) == 0
    # another tile count on the same counters: no word of the block holds a ticket of the launches above
    last = Conv("cnt.last", 3, 96, 192, 7, 19)
    for algo in ids:
        y = last.call("res", algo, 3)
        assert torch.equal(y, last.ref32("res")[0]), (algo, _first_diff(y, last.ref32("res")[0]))
    assert ops.splitk_counters(dev) is cnt and int(cnt.abs().sum()) == 0


# ---- GELU forms at an exactly known pre-activation --------------------------------------------------------------------------------------
def _grid():
    return torch.arange(-640, 641, dtype=torch.float32) / 64.0  # the multiples of 1/64 in [-10, 10]


def _host_figures(z):
    """(GELU, GELU') worst error of torch's fp32 evaluation on the CPU, over the multiples of 1/64 in [-10, 10] and the test's own z"""
    zs = torch.cat([_grid(), z.detach().cpu().float().reshape(-1)])
    return R.host_units(R.gelu32, R.gelu, zs, R.gelu_unit), R.host_units(R.gelu_grad32, R.gelu_grad, zs, R.grad_unit)


def test_conv_cn_gelu_forms_at_exact_preactivation():
    """Codes 2 and 3 and code 0 + dact_z on every id that takes them, n on both store widths.  Operands in eighths, the shift a multiple
    of 1/64: z is exact, `second` of code 2 must equal it bit for bit, and y, GELU'(z) and the dact_z product are compared per element
    with fp64 at that z.  Allowed: 4 x the host's own worst error (see the module docstring for the figures seen).  The dact_z product
    v * GELU'(zt) with an exact v: |v| * (4 x host GELU' units + |GELU'(zt)|) * 2^-24 -- the factor's error and the product's rounding."""
    _, mgfn_ops, _ = _mods()
    bad, worst = [], {"gelu.y": 0.0, "gelu_d.y": 0.0, "gelu_d.second": 0.0, "dact.y": 0.0, "pair.y": 0.0, "pair.second": 0.0}
    cin, cout = 64, 128
    for n in (63, 64, 129, 132):
        zt = R.eighths(f"ge.zt{n}", (cout, 1, n), -4, 4)
        case = Conv(f"ge.{n}", 1, cin, cout, 1, n, maker=R.eighths, dact=zt)
        case.shift = R.ints(f"ge.s{n}", (cout,), -32, 32) / 64.0
        case.d["shift"] = case.shift.to(DEV)
        z64 = R.conv_cn_ref(case.x, case.w, 1, shift=case.shift)[0]
        assert torch.equal(z64.float().double(), z64) and float(z64.abs().max()) > 6
        hg, hd = _host_figures(torch.cat([z64.reshape(-1), zt.reshape(-1).double()]))
        z32, ug, gz = z64.float().to(DEV), R.gelu_unit(z64).to(DEV), R.gelu(z64).to(DEV)
        dz, v64 = R.gelu_grad(z64).to(DEV), R.conv_acc(case.x, case.w, 1) + case.shift.double().reshape(cout, 1, 1)
        gzt = R.gelu_grad(zt)
        dact_ref, dact_bound = (v64 * gzt).to(DEV), (v64.abs() * (4 * hd + gzt.abs()) * U24 * (1 + 2.0 ** -20)).to(DEV)
        # act_gelu_grad(z) itself: a launch whose accumulator is exactly 1 times GELU'(dact_z = z)
        one = Conv(f"ge.one{n}", 1, 32, cout, 1, n, maker=lambda name, shape: torch.zeros(shape), dact=z64.float())
        one.x[0] = 1.0
        one.w[:, 0] = 1.0
        one.xd, one.wd = R.embed(one.x, 64, NAN, device=DEV), one.w.to(DEV)

        g_default = one.call("dact").double()  # act_gelu_grad(z) as the default tile computes it

        def check(pend):
            out, stats = [], []
            for what, algo, fam, form, s, y, second in pend:
                yd = y.double()
                if form == "gelu":
                    stats.append([((yd - gz).abs() / ug).max(), (second != z32).any().double()])
                elif form == "gelu_d":
                    # the pair it replaces: code 2's y and act_gelu_grad(z), of the same id where that id takes a dact_z operand
                    takes_dact = _expected_refusal(algo, 1, 32, cout, n, "dact", 1, True) is None
                    g = one.call("dact", algo, 1).double() if takes_dact else g_default
                    y2 = case.call("gelu", algo, 1)[0].double()
                    stats.append([((yd - gz).abs() / ug).max(), ((second.double() - dz).abs() / U24).max(),
                                  ((yd - y2).abs() / ug).max(), ((second.double() - g).abs() / U24).max()])
                    if _expected_refusal(algo, 1, cin, cout, n, "mul", 1, True) is None:
                        # the same instructions: the stored derivative times an exact accumulator, on the device and formed here in fp32
                        y4 = mgfn_ops.conv_cn(case.xd, case.pack(algo), cout, 1, shift=case.d["shift"], act=R.ACT_MUL, dact_z=second, algo=algo, splits=1)
                        stats[-1].append((y4 != z32 * second).any().double())
                else:
                    stats.append([((yd - dact_ref).abs() / dact_bound.clamp_min(1e-300)).max()])
            vals = [torch.stack(st).cpu().tolist() for st in stats]
            for (what, algo, fam, form, s, y, second), v in zip(pend, vals):
                if form == "gelu":
                    worst["gelu.y"] = max(worst["gelu.y"], v[0])
                    ok = v[0] <= 4 * hg and v[1] == 0
                elif form == "gelu_d":
                    for name, x in zip(("gelu_d.y", "gelu_d.second", "pair.y", "pair.second"), v):
                        worst[name] = max(worst[name], x)
                    ok = v[0] <= 4 * hg and v[1] <= 4 * hd and v[2] <= 4 * hg and v[3] <= 4 * hd and all(x == 0 for x in v[4:])
                else:
                    worst["dact.y"] = max(worst["dact.y"], v[0])  # (a fraction of its bound)
                    ok = v[0] <= 1.0
                if not ok or any(x != x for x in v):
                    out.append(f"{what}: {v} (host GELU {hg:.2f}, GELU' {hd:.2f} units; allowed 4 x)")
                else:
                    RAN.add((fam, form, n % 4 == 0))
                    EPI.add((_epilogue_body(algo, form, s), n % 4 == 0))
            return out

        bad += _sweep(case, GELU_FORMS, check=check)
        print(f"FIGURES conv n={n}: host GELU {hg:.3f} GELU' {hd:.3f} units; device worst so far {worst}")
    assert not bad, f"{len(bad)} complaints, the first 20:\n" + "\n".join(bad[:20])


# ---- real-valued accumulation, element-wise -----------------------------------------------------------------------------------------------
def test_conv_cn_dense_floats_stay_inside_the_derived_bound_per_element():
    """Dense floats, K = 64, every id: |y - ref| <= 2 (K + 4) 2^-24 (sum_k |a_k||b_k| + |shift| + |res|) per element -- K + 4 roundings of
    at most 2^-24 relative each (the epilogue's included), doubled for an MFMA accumulate that need not round to nearest.  The split-bf16
    family drops the lo * lo term and rounds lo to 8 bits: each product is off by at most 3 x 2^-18 < 2^-16 relative on top of that."""
    cin, cout = 64, 128
    bad = []
    for n in (129, 132):
        mk = lambda name, shape: synth_tensor(name, shape, scale=1.5)  # noqa: E731
        case = Conv(f"rv.{n}", 1, cin, cout, 1, n, maker=mk)
        ref = case.ref64("res")[0].to(DEV)
        mag = (R.conv_acc(case.x.abs(), case.w.abs(), 1) + case.shift.abs().double().reshape(cout, 1, 1) + case.res.abs().double()).to(DEV)

        def check(pend):
            out = []
            ex = torch.stack([((y.double() - ref).abs() / (mag * (2 * (cin + 4) * U24 + (2.0 ** -16 if fam == "bf16x3" else 0.0)))).max()
                              for what, algo, fam, form, s, y, z in pend]).cpu().tolist()
            for (what, algo, fam, form, s, y, z), e in zip(pend, ex):
                if not e <= 1.0:
                    i = int(((y.double() - ref).abs() / mag).reshape(-1).argmax())
                    out.append(f"{what}: {e:.3f} of the bound at element {i}: got {float(y.reshape(-1)[i])!r}, want {float(ref.reshape(-1)[i])!r}")
            return out

        bad += _sweep(case, ("res",), check=check)
    assert not bad, f"{len(bad)} complaints, the first 20:\n" + "\n".join(bad[:20])


def test_every_form_ran_on_both_branches_or_was_refused_as_documented():
    """What the tests above recorded: every (family, form) that does not refuse returned the reference on both
    store widths, every refusal carried a documented text, and each of the six pipelined epilogue bodies and the generic one ran on the
    16-byte (n % 4 == 0) and on the scalar (n % 4 != 0) branch."""
    if not SEEN:  # selected on its own: the sweeps that record, at one parameter set each
        test_conv_cn_k1_every_id_and_form_equals_the_integers(64, 128)
        test_conv_cn_k3_taps_are_masked_at_both_ends_of_every_sequence(32, 64)
        test_conv_cn_split_k_returns_the_same_integers(3, 96, (2, 3), ((5, 13), (2, 32)))
        test_conv_cn_gelu_forms_at_exact_preactivation()
    fams = {info[0] for info in _algos().values()}
    assert fams == {"generic", "fast", "dma3", "dma4", "bf16x3", "dma2", "tspan", "mixed", "persist", "tfold"}
    assert SEEN == {(fam, form) for fam in fams for form in FORMS}, sorted({(fam, form) for fam in fams for form in FORMS} - SEEN)
    ran = {(fam, form) for fam, form, _vw in RAN}
    refused = {(fam, form) for fam, form, _why in REFUSED}
    print("RAN (family, form, n % 4 == 0):", sorted(RAN))
    print("REFUSED (family, form, text):", sorted(REFUSED))
    print("EPILOGUES (body, n % 4 == 0):", sorted(EPI))
    assert ran | refused == SEEN, sorted(SEEN - ran - refused)
    missing = sorted((fam, form, vw) for fam, form in ran for vw in (True, False) if (fam, form, vw) not in RAN)
    # the one exemption: the persistent kernels take 16-byte aligned rows only, and rows of another length count as such only when no extra
    # operand is there (they are padded in the index space) -- with a second output they run on n % 4 == 0 alone
    assert missing == sorted(("persist", f, False) for f in FORMS if FORMS[f].get("preact") and not FORMS[f].get("dact")), missing
    # never-running pairs are exactly the documented ones: TSPAN (no (kt,1,1) conv on an even number of frames here) and the families
    # without the extra operands
    never = SEEN - ran
    assert {fam for fam, _form in never} <= {"tspan", "mixed", "persist", "tfold"}, sorted(never)
    assert {(fam, form) for fam, form in never if fam == "mixed"} == {("mixed", f) for f in FORMS if FORMS[f].get("ln") or FORMS[f].get("dact") or FORMS[f].get("preact")}
    assert {(fam, form) for fam, form in never if fam == "persist"} == {("persist", f) for f in FORMS if FORMS[f].get("ln") or FORMS[f].get("dact")}
    assert {(fam, form) for fam, form in never if fam == "tfold"} == {("tfold", f) for f in FORMS if FORMS[f].get("ln")}
    assert {(fam, form) for fam, form in never if fam == "tspan"} == {("tspan", f) for f in FORMS}
    bodies = ("EM_PLAIN", "EM_RES", "EM_DACT", "EM_GELU", "EM_MUL", "EM_GELU2", "generic")
    assert not [(b, vw) for b in bodies for vw in (True, False) if (b, vw) not in EPI], sorted(EPI)
    assert ("split-K", True) in EPI and ("split-K", False) in EPI


# ---- gemm_nt family -------------------------------------------------------------------------------------------------------------------------
NT_SIZES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
NT_PAIRS = tuple((NT_SIZES[i], NT_SIZES[(i + 3) % 10]) for i in range(10))  # each size once as M and once as N


def _nt_refs(tag, M, N, K, pitch=None, offset=0):
    a, b = R.ints(tag + ".a", (M, K)), R.ints(tag + ".b", (N, K))
    p, rs = R.gemm_nt_ref(a, b)
    return (R.embed(a, 64, NAN, offset, pitch, DEV), R.embed(b, 64, NAN, offset, pitch, DEV), p.float().to(DEV), rs.float().to(DEV))


@pytest.mark.parametrize("M,N", NT_PAIRS)
def test_gemm_nt_every_form_tile_and_split_equals_the_integers(M, N):
    """advhip_gemm_nt_f32 / _rowsum_f32 (slices summed here), the slab form + advhip_sum_slabs_f32 and the in-launch reduction, tiles 1-3,
    1 / 2 / 3 / K/16 slices: product and row sums equal the fp64 integers -- and so each other -- with the operands inside NaN."""
    _lib, _, ops = _mods()
    lib, st = _lib.load(), _lib.stream(torch.device(DEV))
    flags, tags = [], []
    for K in (16, 32, 48, 272):
        a, b, p, rs = _nt_refs(f"nt.{M}.{N}.{K}", M, N, K)
        for tile in (1, 2, 3):
            for s in sorted({s for s in (1, 2, 3, K // 16) if s <= K // 16}):
                c, r = torch.full((s, M, N), NAN, device=DEV), torch.full((s, M), NAN, device=DEV)
                _lib.check(lib.advhip_gemm_nt_rowsum_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), r.data_ptr(), M, N, K, K, K, N, s, M * N, tile, st), "gemm_nt_rowsum")
                outs = [("rowsum", c.sum(0), r.sum(0))]
                if tile == 1:
                    c0 = torch.full((s, M, N), NAN, device=DEV)
                    _lib.check(lib.advhip_gemm_nt_f32(a.data_ptr(), b.data_ptr(), c0.data_ptr(), M, N, K, K, K, N, s, M * N, st), "gemm_nt")
                    outs.append(("plain", c0.sum(0), rs))
                if s > 1:
                    outs.append(("slabs",) + tuple(ops.gemm_nt(a, b, splits=s, rowsum=True, tile=tile, reduce_in_kernel=False)))
                outs.append(("reduced",) + tuple(ops.gemm_nt(a, b, splits=s, rowsum=True, tile=tile, reduce_in_kernel=True)))
                outs.append(("reduced, no row sums", ops.gemm_nt(a, b, splits=s, tile=tile, reduce_in_kernel=True), rs))
                for name, gp, gr in outs:
                    flags.append((gp != p).any() | (gr != rs).any())
                    tags.append(f"K={K} tile {tile} splits {s} {name}")
    wrong = [t for t, f in zip(tags, torch.stack(flags).cpu().tolist()) if f]
    assert not wrong, wrong[:20]
    for ws in ops._ZERO_WORKSPACES.values():  # the arrival counters of the in-launch reduction: left zero
        assert int((ws[:16384] != 0).sum()) == 0


def test_gemm_nt_group_of_more_than_32_items_equals_the_integers():
    _, _, ops = _mods()
    for K in (48, 272):
        items, refs = [], []
        for i in range(35):
            M, N = NT_PAIRS[i % 10] if i % 3 else (NT_SIZES[i % 10], NT_SIZES[(i * 7 + 1) % 10])
            a, b, p, rs = _nt_refs(f"ntg.{K}.{i}", M, N, K, pitch=K + 4 * (i % 3))
            items.append((a, b, i % 2 == 0))
            refs.append((p, rs))
        outs = ops.gemm_nt_group(items)
        flags = [(gp != p).any() | ((gr != rs).any() if rsum else torch.zeros((), dtype=torch.bool, device=DEV))
                 for (gp, gr), (p, rs), (_a, _b, rsum) in zip(outs, refs, items)]
        assert all((gr is None) == (not rsum) for (_gp, gr), (_a, _b, rsum) in zip(outs, items))
        wrong = [i for i, f in enumerate(torch.stack(flags).cpu().tolist()) if f]
        assert not wrong, (K, wrong)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_sum_slabs_batches_of_eight_and_their_tail(n):
    _lib = _mods()[0]
    lib, st = _lib.load(), _lib.stream(torch.device(DEV))
    for s in (1, 2, 8, 9, 10, 17):
        stride = n + 3
        src = R.ints(f"ss.{n}.{s}", (s, stride), -50, 50)
        srcd = R.embed(src, 64, NAN, device=DEV)
        out = R.embed(torch.zeros(n), 64, SENT, device=DEV)
        _lib.check(lib.advhip_sum_slabs_f32(srcd.data_ptr(), out.data_ptr(), n, s, stride, st), "sum_slabs")
        assert torch.equal(out.cpu(), src[:, :n].double().sum(0).float()), (n, s)
        assert bool((R.outside(out) == SENT).all())


@pytest.mark.parametrize("pitch_extra", [0, 1, 33])
def test_gemm_nt_operand_placement_through_the_c_abi(pitch_extra):
    """Row pitches K, K + 1, K + 33 (odd ones: the scorer's 2 049-float rows), bases on 4-, 8- and 16-byte alignment, operands inside NaN;
    the output with ldc = N + 5 inside a sentinel buffer whose spare columns stay, slab strides above M * ldc whose gaps stay."""
    _lib = _mods()[0]
    lib, st = _lib.load(), _lib.stream(torch.device(DEV))
    M, N, K = 65, 17, 48
    for offset in (0, 1, 2):
        a, b, p, rs = _nt_refs(f"ntp.{pitch_extra}.{offset}", M, N, K, pitch=K + pitch_extra, offset=offset)
        assert a.data_ptr() % 16 == 4 * offset and a.stride(0) == K + pitch_extra
        lda = ldb = K + pitch_extra
        ldc = N + 5
        for tile in (1, 2, 3):
            for s in (1, 3):
                slab = M * ldc + 7
                buf = torch.full((64 + s * slab + 64,), SENT, device=DEV)
                c = buf.as_strided((s, M, N), (slab, ldc, 1), 64)
                r = R.embed(torch.zeros(s, M), 64, SENT, device=DEV)
                _lib.check(lib.advhip_gemm_nt_rowsum_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), r.data_ptr(), M, N, K, lda, ldb, ldc, s, slab, tile, st), "gemm_nt_rowsum")
                assert torch.equal(c.sum(0), p) and torch.equal(r.sum(0), rs), (offset, tile, s)
                assert bool((R.outside(c) == SENT).all()) and bool((R.outside(r) == SENT).all()), (offset, tile, s)
                # the in-launch reduction writes C (pitch ldc) and the row sums once
                cr = R.embed(torch.zeros(M, N), 64, SENT, pitch=ldc, device=DEV)
                rr = R.embed(torch.zeros(M), 64, SENT, device=DEV)
                need = lib.advhip_gemm_nt_workspace_bytes(M, N, s, tile)
                ws = torch.zeros((max(need, 4) // 4,), device=DEV)
                _lib.check(lib.advhip_gemm_nt_reduced_f32(a.data_ptr(), b.data_ptr(), cr.data_ptr(), rr.data_ptr(), M, N, K, lda, ldb, ldc, s, tile,
                                                          ws.data_ptr() if s > 1 else None, need, st), "gemm_nt_reduced")
                assert torch.equal(cr, p) and torch.equal(rr, rs), (offset, tile, s)
                assert bool((R.outside(cr) == SENT).all()) and bool((R.outside(rr) == SENT).all()), (offset, tile, s)
                assert int((ws[:16384] != 0).sum()) == 0


def test_gemm_nt_refusals_come_with_the_launchers_message_and_write_nothing():
    _lib = _mods()[0]
    lib, st = _lib.load(), _lib.stream(torch.device(DEV))
    M, N, K = 17, 15, 32
    a, b = torch.zeros((M, 64), device=DEV), torch.zeros((N, 64), device=DEV)
    c = torch.full((4, M, N + 8), SENT, device=DEV)
    r = torch.full((4, M), SENT, device=DEV)
    ws = torch.zeros((lib.advhip_gemm_nt_workspace_bytes(M, N, 2, 1) // 4,), device=DEV)
    ap, bp, cp, rp = a.data_ptr(), b.data_ptr(), c.data_ptr(), r.data_ptr()

    def refused(rc, text):
        msg = lib.advhip_last_error().decode()
        assert rc == -1 and re.search(text, msg), (rc, msg, text)

    refused(lib.advhip_gemm_nt_rowsum_f32(ap, bp, cp, rp, M, N, 24, 64, 64, N, 1, M * N, 1, st), "K=24 must be a multiple of 16")
    refused(lib.advhip_gemm_nt_rowsum_f32(ap, bp, cp, rp, M, N, K, 64, 64, N, 3, M * N, 1, st), "bad split count 3")
    refused(lib.advhip_gemm_nt_rowsum_f32(ap, bp, cp, rp, M, N, K, K - 1, 64, N, 1, M * N, 1, st), "row pitch smaller than a row")
    refused(lib.advhip_gemm_nt_rowsum_f32(ap, bp, cp, rp, M, N, K, 64, K - 4, N, 1, M * N, 1, st), "row pitch smaller than a row")
    refused(lib.advhip_gemm_nt_rowsum_f32(ap, bp, cp, rp, M, N, K, 64, 64, N - 1, 1, M * N, 1, st), "row pitch smaller than a row")
    refused(lib.advhip_gemm_nt_rowsum_f32(ap, bp, cp, rp, M, N, K, 64, 64, N, 1, M * N, 4, st), "tile id 4")
    refused(lib.advhip_gemm_nt_f32(ap, bp, cp, M, N, K, 64, 64, N, 2, M * N - 1, st), "bad split count 2")  # (slabs that would overlap)
    refused(lib.advhip_gemm_nt_reduced_f32(ap, bp, cp, rp, M, N, K, 64, 64, N, 2, 1, None, 0, st), "K slices need a workspace")
    refused(lib.advhip_gemm_nt_reduced_f32(ap, bp, cp, rp, M, N, K, 64, 64, N, 2, 1, ws.data_ptr(), ws.numel() * 4 - 4, st), "needs a 256-byte aligned workspace")
    refused(lib.advhip_gemm_nt_reduced_f32(ap, bp, cp, rp, M, N, K, 64, 64, N, 2, 1, ws.data_ptr() + 16, ws.numel() * 4, st), "needs a 256-byte aligned workspace")
    for A, lda in ((ap + 4, 64), (ap, 65), (ap + 8, 64)):  # a group item on a 4- / 8-byte base, or with a pitch that is no multiple of 4
        items = (_lib.NtItem * 2)()
        for it, aa, la in zip(items, (ap, A), (64, lda)):
            it.A, it.B, it.C, it.rowsum, it.M, it.N, it.lda, it.ldb = aa, bp, cp, None, M - 1, N, la, 64
        refused(lib.advhip_gemm_nt_group_slabs_f32(items, 2, K, 1, M * (N + 8), st), "item 1: operands must be 16-byte aligned with row pitches that are multiples of 4")
    torch.cuda.synchronize()
    assert bool((c == SENT).all()) and bool((r == SENT).all()) and int((ws != 0).sum()) == 0


# ---- bgemm --------------------------------------------------------------------------------------------------------------------------------
def _operand(t, kc, offset=0, extra=0):
    """`t` (batch, rows, K) on the device inside NaN: k-contiguous (pitch K + extra), or stored (batch, K, rows) and viewed transposed"""
    if kc:
        return R.embed(t, 64, NAN, offset, t.shape[-1] + extra if extra else None, DEV)
    s = t.transpose(1, 2).contiguous()
    return R.embed(s, 64, NAN, offset, s.shape[-1] + extra if extra else None, DEV).transpose(1, 2)


def _out_like(batch, M, N, how, values=None):
    """an output (or residual) view of shape (batch, M, N) inside a sentinel buffer: dense, pitched rows, transposed, or a row slice"""
    v = torch.zeros((batch, M, N)) if values is None else values
    if how == "dense":
        return R.embed(v, 64, SENT, device=DEV)
    if how == "pitched":
        return R.embed(v, 64, SENT, pitch=N + 3, device=DEV)
    if how == "transposed":
        return R.embed(v.transpose(1, 2).contiguous(), 64, SENT, pitch=M + 1, device=DEV).transpose(1, 2)
    big = torch.full((batch, M + 5, N), SENT)
    big[:, 2 : 2 + M] = v
    return R.embed(big, 64, SENT, device=DEV)[:, 2 : 2 + M]


BGEMM_VARIANTS = (
    dict(alpha=1.0), dict(alpha=2.0, bias_m=True, act=1), dict(alpha=0.5, bias_n=True, residual=True, beta=1.0),
    dict(alpha=1.0, bias_m=True, bias_n=True, residual=True, beta=-2.0), dict(alpha=1.0, ln=True, bias_m=True),
    dict(alpha=2.0, ln=True, act=1, residual=True, beta=1.0),
)
OUT_FORMS = ("dense", "pitched", "transposed", "slice")


def _bgemm_case(tag, a_kc, b_kc, batch, a_batch, M, N, K, variant, out_how, offset, extra, maker=R.ints):
    _, _, ops = _mods()
    a, b = maker(tag + ".a", (a_batch, M, K)), maker(tag + ".b", (batch, K, N))
    ad, bd = _operand(a, a_kc, offset, extra), _operand(b.transpose(1, 2), b_kc, offset, extra).transpose(1, 2)
    v = BGEMM_VARIANTS[variant]
    bm = maker(tag + ".bm", (M,)) if v.get("bias_m") else None
    bn = maker(tag + ".bn", (N,)) if v.get("bias_n") else None
    res = maker(tag + ".r", (batch, M, N)) if v.get("residual") else None
    ln = (R.ints(tag + ".u", (M,)), R.ints(tag + ".mu", (batch * N,), -2, 2), 2.0 ** R.ints(tag + ".rs", (batch * N,), -2, 1)) if v.get("ln") else None
    ref = R.bgemm_ref(a, b, alpha=v["alpha"], bias_m=bm, bias_n=bn, act=v.get("act", 0), residual=res, beta=v.get("beta", 1.0), ln=ln)
    out = _out_like(batch, M, N, out_how)
    resd = _out_like(batch, M, N, out_how, res) if res is not None else None
    got = ops.bgemm(ad, bd, alpha=v["alpha"], bias_m=None if bm is None else bm.to(DEV), bias_n=None if bn is None else bn.to(DEV), act=v.get("act", 0),
                    residual=resd, beta=v.get("beta", 1.0), ln=None if ln is None else tuple(q.to(DEV) for q in ln), out=out)
    assert got.data_ptr() == out.data_ptr()
    return out, ref


@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
def test_bgemm_layouts_edges_and_epilogues_equal_the_integers(a_kc, b_kc):
    """All four operand layouts on the 64-row tile: K of 1..33 (K % 4 != 0 on aligned bases; K % 4 == 0 on a 4-byte base or an odd pitch:
    the 16-byte loads of a k-contiguous operand on and off), M / N around the tiles, a broadcast A, alpha 1 / 2 / 0.5, both biases, ReLU,
    beta 1 / -2 with a residual, the LayerNorm fold with power-of-two rs; outputs and residuals dense, pitched, transposed and as a row
    slice inside a sentinel buffer."""
    pend, i = [], 0
    for M, N in ((63, 65), (64, 129), (65, 64), (129, 63)):
        for K in (1, 3, 4, 5, 15, 16, 17, 33):
            for variant in range(len(BGEMM_VARIANTS)):
                i += 1
                offset, extra = ((0, 0), (1, 0), (0, 1), (0, 4))[(i // 2) % 4]
                how = OUT_FORMS[i % 4]
                out, ref = _bgemm_case(f"bg.{a_kc}{b_kc}.{M}.{N}.{K}.{variant}", a_kc, b_kc, 2, 1 if i % 3 == 0 else 2, M, N, K, variant, how, offset, extra)
                assert torch.equal(ref.float().double(), ref)
                pend.append((f"M={M} N={N} K={K} variant {variant} out {how} offset {offset} pitch +{extra}", out, ref.float().to(DEV), how))
    flags = torch.stack([(out != ref).any() for _t, out, ref, _h in pend]).cpu().tolist()
    wrong = [f"{t}: {_first_diff(out, ref)}" for (t, out, ref, _h), f in zip(pend, flags) if f]
    assert not wrong, f"{len(wrong)} wrong, the first 10:\n" + "\n".join(wrong[:10])
    for t, out, ref, how in pend:
        assert bool((R.outside(out) == SENT).all()), t


@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
def test_bgemm_128_row_tile_equals_the_integers(a_kc, b_kc):
    """ceil(M/64) ceil(N/64) batch >= 4096 with M >= 128 picks the 128-row tile: M = 129, N = 65, batch = 683"""
    M, N, batch = 129, 65, 683
    assert -(-M // 64) * -(-N // 64) * batch >= 4096
    for K, variant, how, offset in ((16, 3, "pitched", 0), (5, 5, "dense", 1), (16, 1, "transposed", 1)):
        out, ref = _bgemm_case(f"bgb.{a_kc}{b_kc}.{K}", a_kc, b_kc, batch, 1 if K == 5 else batch, M, N, K, variant, how, offset, 0)
        refd = ref.float().to(DEV)
        assert torch.equal(out, refd), (K, variant, how, _first_diff(out, refd))
        assert bool((R.outside(out) == SENT).all())


def test_bgemm_gelu_at_exact_preactivation():
    _, _, ops = _mods()
    worst = 0.0
    for (M, N, K), (a_kc, b_kc) in zip(((65, 63, 33), (64, 129, 16), (129, 65, 17), (63, 64, 64)), ((True, True), (True, False), (False, True), (False, False))):
        tag = f"bgg.{M}.{N}.{K}"
        a, b, bm = R.eighths(tag + ".a", (2, M, K)), R.eighths(tag + ".b", (2, K, N)), R.ints(tag + ".bm", (M,), -64, 64) / 64.0
        z = R.bgemm_ref(a, b, alpha=0.5, bias_m=bm)
        assert torch.equal(z.float().double(), z)
        hg, _ = _host_figures(z)
        got = ops.bgemm(_operand(a, a_kc), _operand(b.transpose(1, 2), b_kc).transpose(1, 2), alpha=0.5, bias_m=bm.to(DEV), act=2)
        units = float(((got.double() - R.gelu(z).to(DEV)).abs() / R.gelu_unit(z).to(DEV)).max())
        worst = max(worst, units)
        print(f"FIGURES bgemm GELU {tag}: device {units:.3f}, host {hg:.3f}, allowed {4 * hg:.3f} units")
        assert units <= 4 * hg, (tag, units, hg)


# ---- softmax_rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 129, 1000, 16384])
def test_softmax_rows_per_element(n):
    """Inputs in eighths and a power-of-two scale: x * scale - max is exact, so what is left is exp, the sum and the division.  Per element,
    relative to fp64: (n_terms + 8) 2^-24 with n_terms = ceil(n / 64) + 6, the longest chain of additions behind a row's sum (one wavefront
    per row: each lane adds its ceil(n / 64) terms, six butterfly steps add the lanes), the 8 for the division, the product and the
    denominator's share of exp's error; plus 4 x the host's own worst fp32 exp error on the arguments that occur.  Every row sums to 1
    within (n + 8) 2^-24."""
    _, _, ops = _mods()
    t = -torch.arange(0, 8 * 16 + 1, dtype=torch.float32) / 16.0  # every argument of exp here: a multiple of 1/16 in [-8, 0]
    h_exp = R.host_units(torch.exp, torch.exp, t, lambda q: U24 * torch.exp(q))
    worst, n_terms = 0.0, -(-n // 64) + 6
    for rows in (1, 3, 4, 5):
        for scale in (1.0, 0.5):
            x = R.eighths(f"sm.{n}.{rows}", (rows, n), -4, 4)
            if n > 1 and rows > 1:
                x[0] = x[0, 0]  # a row of equal entries
            if n > 1:
                x[-1] = 0.0
                x[-1, n // 2] = 200.0 / scale  # one entry far above the rest
            ref = R.softmax_ref(x, scale).to(DEV)
            xd = R.embed(x, 64, NAN, device=DEV)
            out = R.embed(torch.zeros(rows, n), 64, SENT, device=DEV)
            ops.softmax_rows(xd, scale, out=out)
            inplace = xd.clone()
            ops.softmax_rows(inplace, scale, out=inplace)
            assert torch.equal(inplace, out) and bool((R.outside(out) == SENT).all())
            # (a value below the smallest normal fp32 may arrive as 0: exp(-200) of the last row)
            rel = float((((out.double() - ref).abs() - 2.0 ** -126).clamp_min(0.0) / ref.clamp_min(1e-300)).max() / U24)
            worst = max(worst, rel)
            assert rel <= n_terms + 8 + 4 * h_exp, (rows, scale, rel, h_exp)
            assert float((out.double().sum(-1) - 1.0).abs().max()) <= (n + 8) * U24
            if n & (n - 1) == 0 and (rows > 1 or n == 1):
                assert bool((out[0] == 1.0 / n).all()), (rows, scale)
            if n > 1:
                want = torch.zeros(n, device=DEV)
                want[n // 2] = 1.0
                assert torch.equal(out[-1], want), (rows, scale)
    print(f"FIGURES softmax n={n}: device worst {worst:.3f} units relative, host exp {h_exp:.3f}, allowed {n_terms + 8 + 4 * h_exp:.3f}")
