"""Edge cases of the MIL head and loss kernels (csrc/mil.hip, csrc/loss.hip) against the plain references of tests/_mil_ref.py:
the tie / NaN order of the top-k in every workgroup shape, `mil_topk_select_split` against two `mil_topk_select` calls, the row
norm's partial lane trips and the exported d_mag branch of its backward, and the loss where a test on smooth random inputs cannot
see it -- the margin term's gradient, saturated and denormal scores, zero score maps, sign(0), and more rows than one pass of the
single-block loops covers.

The order of the top-k is the kernel's documented one (NaN first, the larger value, the lower index; DESIGN.md, "MIL top-k
order").  `torch.topk` breaks ties differently and is not the reference here."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from anomaly_detection_on_video_amd.weights import synth_tensor
import _mil_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
KEEP = np.float32(1 / 0.3)  # a surviving element of dropout(p = 0.7)

# T -> pairs (lo, hi) of equal maxima that the scan or the reduction does not meet in index order.  mil_topk_kernel runs 1 wave
# for T <= 2048, 4 waves (256 threads) up to 32768, 16 waves (1024 threads) above: (63, 64) are neighbouring lanes across the row
# wrap (or the last lane of wave 0 and the first of wave 1), (t, t + threads) the same thread, (70, 300) / (70, 1068) thread 44 of
# wave 0 on its second trip against wave 1, the last pair the row's ends.
REGIMES = {
    3: [(0, 2), (1, 2)],  # k = T
    32: [(3, 20), (30, 31), (0, 31)],  # lanes with no candidate
    65: [(63, 64), (0, 64), (7, 40)],  # lane 0 holds t = 0 and t = 64
    2048: [(63, 64), (5, 69), (1, 2047)],
    2049: [(63, 64), (10, 266), (70, 300), (255, 256), (2, 2048)],
    32769: [(63, 64), (10, 1034), (70, 1068), (1023, 1024), (2000, 32768)],
}
TS = sorted(REGIMES)


def _ks(T, *ks):
    return sorted({min(k, T) for k in ks})


@functools.lru_cache(maxsize=None)
def _topk_operands(n, T, ncrops, F):
    feats = synth_tensor(f"edge.f.{T}", (n * ncrops, T, F))
    sc = synth_tensor(f"edge.s.{T}", (n, T), scale=0.5, offset=0.5)
    return feats, sc


@functools.lru_cache(maxsize=None)
def _noise(T, rows=3):
    """(rows, T) magnitudes in [0.1, 1): distinct-looking, positive, below every planted maximum.  Callers copy."""
    return synth_tensor(f"edge.mag.{T}", (rows, T), scale=0.45, offset=0.55).numpy()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def check_topk(mag, keep, k, ncrops=2):
    """One mil_topk_select call forward and backward, everything against tests/_mil_ref.py.  -> idx (n, k) as numpy."""
    from anomaly_detection_on_video_amd import mil_ops

    mag = np.ascontiguousarray(mag, dtype=np.float32)
    keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.float32)
    n, T = mag.shape
    F = 8 if T % 2 == 0 else 5  # the float4 and the scalar path of the gather
    feats, sc = _topk_operands(n, T, ncrops, F)
    idx_r, sel_r, score_r = ref.select(feats, sc, mag, keep, ncrops, k)
    fg = feats.to(DEV).requires_grad_(True)
    sg = sc.to(DEV).requires_grad_(True)
    kp = None if keep is None else torch.from_numpy(keep).to(DEV)
    idx, sel, score = mil_ops.mil_topk_select(torch.from_numpy(mag).to(DEV), kp, sg, fg, ncrops, k)
    got = idx.cpu().numpy()
    assert got.shape == (n, k) and sel.shape == (ncrops * n, k, F) and score.shape == (n, 1)
    assert np.array_equal(got, idx_r), f"T={T} k={k}: idx {got.tolist()} != {idx_r.tolist()}"
    assert all(len(set(row.tolist())) == k for row in got)  # what makes the backward scatter race-free
    assert torch.equal(_bits(sel), _bits(torch.from_numpy(sel_r)))  # a gather: bit for bit
    assert rel_err(score.detach().cpu().view(-1), score_r) < 1e-5
    d_sel = synth_tensor(f"edge.dsel.{T}.{k}", tuple(sel.shape))
    d_score = synth_tensor(f"edge.dscore.{T}", (n, 1), scale=1.0, offset=2.0)
    torch.autograd.backward([sel, score], [d_sel.to(DEV), d_score.to(DEV)])
    d_f, d_s = ref.select_bwd(idx_r, d_sel, d_score, (n, ncrops, T, F, k))
    assert torch.equal(fg.grad.cpu(), torch.from_numpy(d_f))  # copies into zeros
    assert torch.equal(sg.grad.cpu(), torch.from_numpy(d_s))  # one fp32 division by k
    return got


# ------------------------------------------------------------------------------------------------ A. top-k order
@pytest.mark.parametrize("T", TS)
def test_topk_all_equal_row_takes_the_first_k(T):
    for k in _ks(T, 1, 3, 16):
        got = check_topk(_noise(T, 2), np.zeros((2, T), np.float32), k)  # every product is +0
        assert got.tolist() == [list(range(k))] * 2
    got = check_topk(np.full((1, T), 1.5, np.float32), None, min(3, T), ncrops=1)  # equal and not zero, no mask
    assert got.tolist() == [list(range(min(3, T)))]


@pytest.mark.parametrize("T", TS)
def test_topk_with_fewer_than_k_survivors_of_the_dropout_mask(T):
    """The training case: dropout(0.7) over T = 32 segments leaves fewer than k = 3 of them once in ~800 videos."""
    for k in _ks(T, 3, 16):
        mag = _noise(T, 3).copy()
        keep = np.zeros((3, T), np.float32)  # row 0: nobody survives
        keep[1, T - 1] = KEEP  # row 1: one survivor, at the end
        keep[2, T - 2:] = KEEP  # row 2: two, the later one larger
        mag[2, T - 2], mag[2, T - 1] = 0.25, 0.75
        got = check_topk(mag, keep, k)
        zeros = list(range(k))
        assert got[0].tolist() == zeros
        assert got[1].tolist() == ([T - 1] + zeros)[:k]
        assert got[2].tolist() == ([T - 1, T - 2] + zeros)[:k]
        mag[2, T - 2] = 0.75  # two equal survivors: by index, then the zeros
        got = check_topk(mag[2:], keep[2:], k, ncrops=3)
        assert got[0].tolist() == ([T - 2, T - 1] + zeros)[:k]


@pytest.mark.parametrize("T", TS)
def test_topk_equal_maxima_the_lower_index_wins(T):
    pairs = REGIMES[T]
    for lo in range(0, len(pairs), 3):
        chunk = pairs[lo : lo + 3]
        mag = _noise(T, 3)[: len(chunk)].copy()
        for r, (a, b) in enumerate(chunk):
            assert a < b < T
            mag[r, a] = mag[r, b] = 2.0
        got = check_topk(mag, None, 1)
        assert got[:, 0].tolist() == [a for a, _ in chunk]
        k = min(3, T)
        got = check_topk(mag, np.full(mag.shape, KEEP, np.float32), k)  # equal products of equal factors
        assert got[:, :2].tolist() == [[a, b] for a, b in chunk]
    # every pair in one row: 2 * len(pairs) equal maxima, fewer than that asked for
    mag = _noise(T, 1).copy()
    where = sorted({t for p in pairs for t in p})
    mag[0, where] = 2.0
    k = min(len(where) - 1, 16)
    assert check_topk(mag, None, k, ncrops=1)[0].tolist() == where[:k]


@pytest.mark.parametrize("T", TS)
def test_topk_nan_comes_first_by_index_then_inf(T):
    mid = T // 2
    for k in _ks(T, 3, 16):
        mag = _noise(T, 3).copy()
        mag[0, T - 1] = NAN  # one NaN
        mag[1, T - 1] = mag[1, mid] = NAN  # two
        mag[2, T - 1], mag[2, mid], mag[2, 0] = NAN, INF, NAN  # NaN above +inf
        got = check_topk(mag, None, k)
        assert got[0, 0] == T - 1
        assert got[1, :2].tolist() == [mid, T - 1]
        assert got[2].tolist()[:3] == [0, T - 1, mid][:k]
        # through the mask: inf * 0 = NaN (row 0), NaN * 0 = NaN among too few survivors (row 1), a masked NaN and a kept +inf (row 2)
        mag = _noise(T, 3).copy()
        keep = np.full((3, T), KEEP, np.float32)
        mag[0, T - 1], keep[0, T - 1] = INF, 0
        mag[0, 0] = INF
        keep[1] = 0
        mag[1, T - 1] = NAN
        keep[1, mid] = KEEP
        mag[2, mid], keep[2, mid] = NAN, 0
        mag[2, T - 1] = INF
        got = check_topk(mag, keep, k)
        assert got[0, :2].tolist() == [T - 1, 0]
        assert got[1].tolist() == ([T - 1, mid] + [t for t in range(k) if t not in (mid, T - 1)])[:k]
        assert got[2, :2].tolist() == [mid, T - 1]


@pytest.mark.parametrize("T", TS)
def test_topk_minus_inf_is_an_ordinary_smallest_value(T):
    k = min(16, T)  # k = T at T = 3: every -inf entry is chosen
    mag = np.full((3, T), -INF, np.float32)  # row 0: nothing else
    mag[1, T - 1] = 1.0  # row 1: one finite entry at the end
    mag[2, T - 1], mag[2, T // 2] = -1.0, NAN  # row 2: NaN, a finite entry, then -inf by index
    got = check_topk(mag, None, k)
    assert got[0].tolist() == list(range(k))
    assert got[1].tolist() == ([T - 1] + list(range(k)))[:k]
    assert got[2].tolist() == ([T // 2, T - 1] + [t for t in range(k + 2) if t not in (T // 2, T - 1)])[:k]
    got = check_topk(mag, np.full((3, T), KEEP, np.float32), min(3, T))  # -inf * keep = -inf
    assert got[0].tolist() == list(range(min(3, T)))


@pytest.mark.parametrize("T", TS)
def test_topk_plus_zero_and_minus_zero_tie(T):
    for k in _ks(T, 3, 16):
        mag = synth_tensor(f"edge.signed.{T}", (2, T)).numpy().copy()  # both signs: the products are +0 and -0
        assert (mag[0] < 0).any() and (mag[0] > 0).any()
        keep = np.zeros((2, T), np.float32)
        # row 1: negative survivors; the masked entries are -0 (at T // 2) and +0 (at T - 1) and lead in index order
        mag[1] = -np.abs(mag[1]) - 0.5
        keep[1] = KEEP
        keep[1, T // 2] = keep[1, T - 1] = 0
        mag[1, T - 1] = 0.5
        got = check_topk(mag, keep, k)
        assert got[0].tolist() == list(range(k))
        assert got[1, :2].tolist() == [T // 2, T - 1]


# ------------------------------------------------------------------------------------------------ B. the split node
def test_topk_select_split_equals_two_topk_select_calls():
    from anomaly_detection_on_video_amd import mil_ops

    bs, ncrops, T, F, k = 4, 3, 32, 20, 3
    h = bs // 2
    feats = synth_tensor("edge.split.f", (bs * ncrops, T, F))
    sc = synth_tensor("edge.split.s", (bs, T), scale=0.5, offset=0.5)
    mag = synth_tensor("edge.split.m", (bs, T), scale=0.45, offset=0.55)
    keep = (synth_tensor("edge.split.k", (2, h, T)) > 0.4).float() * float(KEEP)
    keep[0, 1] = 0  # abnormal half, video 1: one survivor
    keep[0, 1, 30] = float(KEEP)
    keep[1, 0] = 0  # normal half, video 0: two
    keep[1, 0, 31] = keep[1, 0, 17] = float(KEEP)
    mag[0, 31], mag[0, 17] = 0.9, 0.2
    keep_a, keep_n = keep[0].to(DEV), keep[1].to(DEV)
    d_outs = [synth_tensor(f"edge.split.d{i}", s) for i, s in enumerate([(ncrops * h, k, F), (h, 1)] * 2)]

    fg, sg = feats.to(DEV).requires_grad_(True), sc.to(DEV).requires_grad_(True)
    mg = mag.to(DEV)
    ia, fa, sa, in_, fn, sn = mil_ops.mil_topk_select_split(mg, keep_a, keep_n, sg, fg, ncrops, k)
    torch.autograd.backward([fa, sa, fn, sn], [d.to(DEV) for d in d_outs])

    # the same on copies of the halves (videos [h, bs) are the abnormal ones), each its own node
    halves = {}
    for name, lo, kp, d_sel, d_score in (("a", h, keep_a, d_outs[0], d_outs[1]), ("n", 0, keep_n, d_outs[2], d_outs[3])):
        f2 = feats[lo * ncrops : (lo + h) * ncrops].clone().to(DEV).requires_grad_(True)
        s2 = sc[lo : lo + h].clone().to(DEV).requires_grad_(True)
        idx, sel, score = mil_ops.mil_topk_select(mag[lo : lo + h].clone().to(DEV), kp, s2, f2, ncrops, k)
        torch.autograd.backward([sel, score], [d_sel.to(DEV), d_score.to(DEV)])
        halves[name] = (idx, sel, score, f2.grad, s2.grad)
        want = ref.select(feats[lo * ncrops : (lo + h) * ncrops], sc[lo : lo + h], mag[lo : lo + h], kp.cpu(), ncrops, k)[0]
        assert np.array_equal(idx.cpu().numpy(), want)
    assert halves["a"][0][1].tolist() == [30, 0, 1] and halves["n"][0][0].tolist() == [31, 17, 0]  # survivors, then the first zeros
    assert torch.equal(ia, halves["a"][0]) and torch.equal(in_, halves["n"][0])
    for got, want in zip((fa, sa, fn, sn), halves["a"][1:3] + halves["n"][1:3]):
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(fg.grad), _bits(torch.cat([halves["n"][3], halves["a"][3]])))
    assert torch.equal(_bits(sg.grad), _bits(torch.cat([halves["n"][4], halves["a"][4]])))


# ------------------------------------------------------------------------------------------------ C. magnitude
def _magnitude_inputs(bs, ncrops, F, T=5):
    feats = synth_tensor(f"edge.mag.f.{F}", (bs * ncrops, T, F))
    feats[bs * ncrops - 1, 2] = 0  # one all-zero row
    scores = synth_tensor(f"edge.mag.s.{F}", (bs * ncrops, T), scale=0.5, offset=0.5)
    return feats, scores


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("ncrops", [1, 3])
@pytest.mark.parametrize("F", [65, 130, 260, 1023])  # a partial second trip of the float4 loop (260) and of the scalar loop
def test_mil_magnitude_forward_vs_float64(F, ncrops, bs):
    from anomaly_detection_on_video_amd import mil_ops

    feats, scores = _magnitude_inputs(bs, ncrops, F)
    mag, sc = mil_ops.mil_magnitude(feats.to(DEV), scores.to(DEV), bs, ncrops)
    mag_r, sc_r = ref.magnitude(feats, scores, bs, ncrops)
    assert rel_err(mag.cpu(), mag_r) < 1e-5
    assert rel_err(sc.cpu(), sc_r) < 1e-5
    if ncrops == 1:
        assert float(mag[bs - 1, 2]) == 0.0


@pytest.mark.parametrize("bs,ncrops", [(1, 1), (2, 3)])
@pytest.mark.parametrize("F", [65, 130, 260, 1023])
def test_mil_magnitude_backward_d_mag_branch_vs_float64_autograd(F, bs, ncrops):
    """The d_mag branch of advhip_mil_magnitude_bwd_f32, which mil_ops never takes (mag is marked non-differentiable there)."""
    from anomaly_detection_on_video_amd import _lib
    from anomaly_detection_on_video_amd._lib import check, ptr, stream

    feats, _ = _magnitude_inputs(bs, ncrops, F)
    rows, T, _ = feats.shape
    d_mag = synth_tensor(f"edge.mag.dm.{F}", (bs, T))
    d_sc = synth_tensor(f"edge.mag.ds.{F}", (bs, T))
    fg = feats.to(DEV)
    for with_sc in (False, True):
        d_feat = torch.zeros_like(fg)  # the kernel accumulates, as in mil_ops
        d_scores = torch.zeros((rows, T), device=DEV) if with_sc else None
        dm, ds = d_mag.to(DEV), (d_sc.to(DEV) if with_sc else None)
        check(_lib.load().advhip_mil_magnitude_bwd_f32(ptr(fg), ptr(dm), ptr(ds), ptr(d_feat), ptr(d_scores), bs, ncrops, T, F, stream()),
              "mil_magnitude_bwd")
        want_f, want_s = ref.magnitude_bwd(feats, d_mag, d_sc if with_sc else None, bs, ncrops)
        got = d_feat.cpu()
        assert not torch.isnan(got).any()
        assert bool((got[rows - 1, 2] == 0).all()) and bool((want_f[rows - 1, 2] == 0).all())  # nrm > 0 ? g / nrm : 0
        assert rel_err(got, want_f) < 1e-5
        if with_sc:
            assert rel_err(d_scores.cpu(), want_s) < 1e-5


# ------------------------------------------------------------------------------------------------ D. loss
def assert_elementwise(got, want, tol, what):
    """max |got - want| / |want| < tol over the entries with want != 0; the others must be exactly zero; nothing is NaN or inf.

    Why not conftest.rel_err, which the reductions are otherwise held to at 1e-5: it divides the largest difference by the largest
    entry, so one large entry hides every small one.  The margin term is 5e-4 of the feature gradient's largest entry at the training shape
    (a flipped sign of it moves test_hip_mgfn.py's norm-wise error to 1.1e-3, a lost clamp to 1.2e-4, next to its 1e-4 bound),
    a saturated score's BCE gradient is 1e12 times its neighbour's, and a row that a strided loop skipped is one entry among
    hundreds: each passes norm-wise while being entirely wrong."""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    want = torch.as_tensor(want).detach().cpu().double().reshape(-1)
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries"
    zero = want == 0
    assert bool((got[zero] == 0).all()), f"{what}: entries that must be exactly zero are not"
    if bool((~zero).any()):
        err = float(((got - want).abs() / want.abs())[~zero].max())
        print(f"{what}: element-wise rel err {err:.3g} (tol {tol:g})")
        assert err < tol, f"{what}: element-wise rel err {err:.3g} >= {tol:g}"


def assert_term(got, want, tol, what):
    got, want = float(got), float(want)
    print(f"{what}: got {got!r} want {want!r}")
    if want == 0:
        assert got == 0, f"{what}: {got!r}, want exactly 0"
    else:
        assert abs(got - want) / abs(want) < tol, f"{what}: {got!r} vs {want!r}"


def run_loss(sc, sa, sn, fa, fn, al, nl, ncrops, g=1.7):
    """-> (terms by name, the five input gradients of g * total) of the HIP loss."""
    from anomaly_detection_on_video_amd import mil_ops

    gpu = [t.to(DEV).requires_grad_(True) for t in (sc, sa, sn, fa, fn)]
    total, t8 = mil_ops.mgfn_loss(*gpu, al.to(DEV), nl.to(DEV), ncrops)
    (total * g).backward()
    terms = dict(zip(mil_ops.LOSS_TERMS, t8.cpu().tolist()))
    assert terms["total"] == float(total.detach())
    return terms, [t.grad.cpu() for t in gpu]


GRADS = ("d_scores", "d_abn", "d_nor", "d_a_feat", "d_n_feat")


def _loss_inputs(tag, n, ncrops, k, F, T):
    bs = 2 * n
    sc = synth_tensor(f"edge.loss.sc.{tag}", (bs, T), scale=0.45, offset=0.5)
    sa = synth_tensor(f"edge.loss.sa.{tag}", (n,), scale=0.4, offset=0.5)
    sn = synth_tensor(f"edge.loss.sn.{tag}", (n,), scale=0.4, offset=0.5)
    fa = synth_tensor(f"edge.loss.fa.{tag}", (ncrops * n, k, F), scale=1.0, offset=0.05)
    fn = synth_tensor(f"edge.loss.fn.{tag}", (ncrops * n, k, F), scale=0.8)
    return sc, sa, sn, fa, fn


@pytest.mark.parametrize("lo,hi", [(160, 200), (240, 330), (160, 330)])
def test_loss_margin_term_gradient_in_isolation(lo, hi):
    """Rows [sep, 2 sep) copy rows [0, sep), so the same-class terms are their 1e-6 epsilon and the feature gradients ARE the
    margin term's: inside the margin (160..200), outside it (con == 0 and no gradient from it), and both."""
    n, ncrops, k, F, T = 2, 2, 3, 40, 4
    sep = n * ncrops // 2

    def rows(name, l1):
        base = synth_tensor(name, (sep, k, F), scale=0.45, offset=0.55).double()  # all positive
        half = (base / base.sum(-1, keepdim=True) * l1).float()
        return torch.cat([half, half])

    fa = rows("edge.margin.a", torch.linspace(lo, hi, sep * k, dtype=torch.float64).view(sep, k, 1))
    fn = rows("edge.margin.n", 100.0)
    assert bool((fa > 0).all()) and bool((fn > 0).all())
    dist = ((fa.double().sum(-1) - fn.double().sum(-1) + 1e-6) ** 2).sum(-1).sqrt()
    assert bool(((dist - 200).abs() >= 10).all()), dist
    inside = dist < 200
    assert bool(inside.all()) == (hi <= 200) and bool((~inside).all()) == (lo >= 240)
    sc, sa, sn, _, _ = _loss_inputs("margin", n, ncrops, k, F, T)
    al, nl = torch.ones(n), torch.zeros(n)
    terms, grads = run_loss(sc, sa, sn, fa, fn, al, nl, ncrops)
    t64, g64 = ref.loss(sc, sa, sn, fa, fn, al, nl, g=1.7)
    assert (t64["con"] == 0) == (lo >= 240)
    assert_term(terms["con"], t64["con"], 1e-5, "con")
    assert_elementwise(grads[3], g64[3], 1e-4, "d_a_feat")
    assert_elementwise(grads[4], g64[4], 1e-4, "d_n_feat")
    # the margin term pulls the abnormal L1 norms up and pushes the normal ones down, only inside the margin
    big = g64[3].abs() > 1e-7
    assert bool((big.reshape(len(dist), -1).all(1) == inside).all())
    assert bool((grads[3][big] < 0).all()) and bool((grads[4][big] > 0).all())


SCORE_VALUES = (0.0, 1.0, 1.0 - 2.0 ** -24, 1e-40, 0.3)


@pytest.mark.parametrize("shift", range(5))
def test_loss_bce_with_saturated_and_denormal_scores(shift):
    """Every (score, label) pair over {0, 1, 1 - 2^-24, 1e-40, 0.3} x {0, 1}, once as an abnormal and once as a normal score."""
    n, ncrops, k, F, T = 2, 2, 3, 8, 4
    combos = [(v, y) for v in SCORE_VALUES for y in (0.0, 1.0)]
    pa = [combos[2 * shift], combos[2 * shift + 1]]
    pn = [combos[(2 * shift + 5) % 10], combos[(2 * shift + 6) % 10]]
    sa, al = (torch.tensor(c, dtype=torch.float32) for c in zip(*pa))
    sn, nl = (torch.tensor(c, dtype=torch.float32) for c in zip(*pn))
    sc, _, _, fa, fn = _loss_inputs("bce", n, ncrops, k, F, T)
    terms, grads = run_loss(sc, sa, sn, fa, fn, al, nl, ncrops, g=1.0)
    t64, g64 = ref.loss(sc, sa, sn, fa, fn, al, nl, g=1.0)
    bce64, gb64 = ref.bce(torch.cat([sn, sa]), torch.cat([nl, al]))
    assert bce64 == pytest.approx(t64["bce"], rel=1e-12) and torch.allclose(gb64, torch.cat([g64[2], g64[1]]), rtol=1e-12, atol=0)
    assert_term(terms["bce"], bce64, 1e-5, "cls")
    assert_elementwise(grads[1], g64[1], 1e-5, "d_abn")
    assert_elementwise(grads[2], g64[2], 1e-5, "d_nor")


def test_loss_bce_clamps_and_the_denormal_score_by_value():
    n, ncrops, k, F, T = 2, 2, 3, 8, 4
    sc, _, _, fa, fn = _loss_inputs("bce", n, ncrops, k, F, T)
    # saturated and wrong: 100 an entry (the logs are clamped at -100), gradients -+ 1 / (1e-12 * 2n)
    sa, al = torch.tensor([0.0, 1.0]), torch.tensor([1.0, 0.0])
    sn, nl = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])
    terms, grads = run_loss(sc, sa, sn, fa, fn, al, nl, ncrops, g=1.0)
    assert_term(terms["bce"], 100.0, 1e-5, "cls, saturated")
    assert_elementwise(grads[1], torch.tensor([-1.0, 1.0], dtype=torch.float64) / (1e-12 * 2 * n), 1e-5, "d_abn, saturated")
    assert_elementwise(grads[2], torch.tensor([1.0, -1.0], dtype=torch.float64) / (1e-12 * 2 * n), 1e-5, "d_nor, saturated")
    # a denormal score is not zero: -log(1e-40) = 92.1, not the clamp's 100
    tiny = torch.tensor([1e-40, 1e-40], dtype=torch.float32)
    assert bool((tiny > 0).all())
    terms, grads = run_loss(sc, tiny, tiny.clone(), fa, fn, torch.ones(n), torch.ones(n), ncrops, g=1.0)
    want = -float(np.log(np.float64(np.float32(1e-40))))
    assert 92.10 < want < 92.11
    assert_term(terms["bce"], want, 1e-5, "cls, denormal")
    assert_elementwise(grads[1], torch.full((n,), -1 / (1e-12 * 2 * n), dtype=torch.float64), 1e-5, "d_abn, denormal")


def _grid_scores(tag, bs, T):
    """Scores on a grid of 1/64 in (0, 1): their differences are exact in fp32, so the smoothness gradient (a difference of
    differences) carries no cancellation error of the inputs and can be held element-wise."""
    s = synth_tensor(f"edge.grid.{tag}.{T}", (bs, T), scale=0.45, offset=0.5)
    return torch.round(s * 64).clamp(1, 63) / 64


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("zero_normal_half", [True, False])
def test_loss_degenerate_score_maps(zero_normal_half, T):
    n, ncrops, k, F = 2, 2, 3, 8
    _, sa, sn, fa, fn = _loss_inputs("degenerate", n, ncrops, k, F, T)
    sc = _grid_scores("degenerate", 2 * n, T)
    if zero_normal_half:
        sc[:n] = 0  # sparse = 8e-3 * ||0|| = 0, whose gradient torch (and the kernel) take as zero
    al, nl = torch.ones(n), torch.zeros(n)
    terms, grads = run_loss(sc, sa, sn, fa, fn, al, nl, ncrops)
    t64, g64 = ref.loss(sc, sa, sn, fa, fn, al, nl, g=1.7)
    assert (t64["sparse"] == 0) == zero_normal_half and (t64["smooth"] == 0) == (T == 1)
    for name in ("smooth", "sparse", "total"):
        assert_term(terms[name], t64[name], 1e-5, name)
    for gr in grads:
        assert bool(torch.isfinite(gr).all())
    assert_elementwise(grads[0], g64[0], 1e-5, "d_scores")
    if zero_normal_half:
        assert not grads[0][:n].any()
    if T == 1 and zero_normal_half:
        assert not grads[0].any()


def test_loss_l1_backward_sign_of_zero():
    n, ncrops, k, F, T = 2, 2, 3, 12, 4
    sc, sa, sn, fa, fn = _loss_inputs("sign0", n, ncrops, k, F, T)
    fa[0, 0, 3], fa[1, 2, 5], fa[3, 1, 11] = 0.0, -0.0, 0.0
    fn[3, 1, 0], fn[2, 0, 11] = -0.0, 0.0
    fa[2, 1] = torch.tensor([0.0, -0.0] * (F // 2))  # a whole row of zeros of both signs
    zero_a, zero_n = fa == 0, fn == 0
    assert int(zero_a.sum()) == 3 + F and int(zero_n.sum()) == 2
    al, nl = torch.ones(n), torch.zeros(n)
    terms, grads = run_loss(sc, sa, sn, fa, fn, al, nl, ncrops)
    t64, g64 = ref.loss(sc, sa, sn, fa, fn, al, nl, g=1.7)
    for got, want, feat, zero, name in ((grads[3], g64[3], fa, zero_a, "d_a_feat"), (grads[4], g64[4], fn, zero_n, "d_n_feat")):
        assert not got[zero].any() and not want[zero].any(), name  # sign(+-0) = 0
        assert bool((got[~zero] != 0).all()), name
        assert rel_err(got, want) < 1e-4, name  # the rest: the existing norm-wise bound (differences of L1 norms cancel in fp32)
        # d l1 / d x = +-1: a row's non-zero entries share one magnitude, with the sign of the feature
        v = got * torch.sign(feat)
        lo = torch.where(zero, torch.full_like(v, INF), v).amin(-1)
        hi = torch.where(zero, torch.full_like(v, -INF), v).amax(-1)
        some = (~zero).any(-1)
        assert torch.equal(lo[some], hi[some]), name
    for name in ("con", "con_a", "con_n", "total"):
        assert_term(terms[name], t64[name], 1e-5, name)


@pytest.mark.parametrize("n,ncrops", [(130, 4), (52, 10)])
def test_loss_rows_beyond_one_pass_of_the_block(n, ncrops):
    """R = 520 and sep = 260 (and 2n = 260 at n = 130): the 256-thread loops of the single-block kernels make a second and a
    third trip.  The gradient buffers are `empty_like`, so a skipped row is an unwritten entry."""
    k, F, T = 3, 8, 3
    sc, sa, sn, fa, fn = _loss_inputs(f"strided.{n}", n, ncrops, k, F, T)
    al = (synth_tensor(f"edge.loss.al.{n}", (n,)) > -0.5).float()  # labels that agree and disagree
    nl = (synth_tensor(f"edge.loss.nl.{n}", (n,)) > 0.5).float()
    assert 0 < al.sum() < n and 0 < nl.sum() < n
    terms, grads = run_loss(sc, sa, sn, fa, fn, al, nl, ncrops)
    t64, g64 = ref.loss(sc, sa, sn, fa, fn, al, nl, g=1.7)
    for name in ref.LOSS_TERMS:
        assert_term(terms[name], t64[name], 1e-5, name)
    for got, want, name in zip(grads, g64, GRADS):
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
        assert rel_err(got, want) < 1e-4, name
    assert_elementwise(grads[1], g64[1], 1e-5, "d_abn")
    assert_elementwise(grads[2], g64[2], 1e-5, "d_nor")
    # every (row, j) of the feature gradients was written: its entries are +-(one magnitude), as in the reference
    for got, want, name in ((grads[3], g64[3], "d_a_feat"), (grads[4], g64[4], "d_n_feat")):
        row_got, row_want = got.abs().amax(-1).double(), want.abs().amax(-1)
        assert float(((row_got - row_want).abs()).max() / row_want.max()) < 1e-4, name
        assert bool((got.abs() == got.abs().amax(-1, keepdim=True)).all()), name
