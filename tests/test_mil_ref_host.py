"""CPU tests of tests/_mil_ref.py, the references that tests/test_hip_mil_edges.py holds the MIL head and loss kernels to."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from anomaly_detection_on_video_amd.weights import synth_tensor
import _mil_ref as ref


@pytest.mark.parametrize("T", [3, 32, 300])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_topk_order_equals_torch_topk_without_ties(T, seed):
    g = torch.Generator().manual_seed(100 * T + seed)
    v = torch.randn((5, T), generator=g)
    assert all(len(set(row.tolist())) == T for row in v), "the draw has a tie"
    for k in {1, min(3, T), min(16, T)}:
        assert np.array_equal(ref.topk_order(v, k), torch.topk(v, k, dim=1).indices.numpy())


def test_topk_order_on_hand_written_rows():
    nan, inf = float("nan"), float("inf")
    for k in (1, 3, 16):
        assert ref.topk_order(np.zeros(32, np.float32), k).tolist() == list(range(k))
    assert ref.topk_order(np.array([0, nan, 2, nan, 2], np.float32), 4).tolist() == [1, 3, 2, 4]
    assert ref.topk_order(np.full(7, -inf, np.float32), 7).tolist() == list(range(7))
    # +0 and -0 are one value; +inf is below NaN and above everything else; -inf is the smallest
    assert ref.topk_order(np.array([-1, -0.0, 0.0, -0.0], np.float32), 3).tolist() == [1, 2, 3]
    assert ref.topk_order(np.array([0.0, -0.0, 5, -0.0], np.float32), 4).tolist() == [2, 0, 1, 3]
    assert ref.topk_order(np.array([1, inf, nan, -inf, inf], np.float32), 5).tolist() == [2, 1, 4, 0, 3]
    # two rows at once
    assert ref.topk_order(np.array([[1, 3, 3], [nan, 0, nan]], np.float32), 2).tolist() == [[1, 2], [0, 2]]


def test_select_and_its_backward_on_a_hand_written_case():
    n, ncrops, T, Fd, k = 2, 2, 4, 3, 2
    feats = np.arange(n * ncrops * T * Fd, dtype=np.float32).reshape(n * ncrops, T, Fd)
    sc = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.6, 0.7, 0.8]])
    mag = np.array([[1, 5, 5, 2], [np.inf, 3, 1, 3]], np.float32)
    keep = np.array([[1, 1, 1, 1], [0, 0, 1, 0]], np.float32)  # second video: inf * 0 = NaN first, then 1, then the zeros
    idx, sel, score = ref.select(feats, sc, mag, keep, ncrops, k)
    assert idx.tolist() == [[1, 2], [0, 2]]
    assert sel.shape == (ncrops * n, k, Fd)
    assert np.array_equal(sel[0], feats[0, [1, 2]]) and np.array_equal(sel[1], feats[2, [0, 2]])  # crop 0 of videos 0, 1
    assert np.array_equal(sel[2], feats[1, [1, 2]]) and np.array_equal(sel[3], feats[3, [0, 2]])  # crop 1
    assert score.tolist() == pytest.approx([0.25, 0.6])
    d_sel = np.arange(sel.size, dtype=np.float32).reshape(sel.shape) + 1
    d_feat, d_sc = ref.select_bwd(idx, d_sel, np.array([3.0, 5.0], np.float32), (n, ncrops, T, Fd, k))
    assert np.array_equal(d_feat[2, [0, 2]], d_sel[1]) and np.array_equal(d_feat[1, [1, 2]], d_sel[2])
    assert d_feat.sum() == d_sel.sum() and np.count_nonzero(d_feat) == d_sel.size
    assert np.array_equal(d_sc, np.array([[0, 1.5, 1.5, 0], [2.5, 0, 2.5, 0]], np.float32))


def test_magnitude_and_its_backward_with_a_zero_row():
    bs, ncrops, T, Fd = 2, 3, 4, 5
    f = synth_tensor("milref.f", (bs * ncrops, T, Fd))
    f[4, 2] = 0
    s = synth_tensor("milref.s", (bs * ncrops, T), scale=0.5, offset=0.5)
    mag, sc = ref.magnitude(f, s, bs, ncrops)
    assert mag.dtype == torch.float64 and mag.shape == (bs, T)
    want = sum(float((f[3 + c, 1].double() ** 2).sum().sqrt()) for c in range(ncrops)) / ncrops
    assert float(mag[1, 1]) == pytest.approx(want, rel=1e-12)
    assert float(sc[0, 3]) == pytest.approx(float(s[:3, 3].double().mean()), rel=1e-12)
    d_mag = synth_tensor("milref.dm", (bs, T))
    d_sc = synth_tensor("milref.ds", (bs, T))
    d_f, d_s = ref.magnitude_bwd(f, d_mag, d_sc, bs, ncrops)
    assert torch.isfinite(d_f).all() and bool((d_f[4, 2] == 0).all())
    r = f[0, 1].double()
    assert torch.allclose(d_f[0, 1], float(d_mag[0, 1]) / ncrops * r / r.norm(), rtol=1e-12, atol=0)
    assert torch.allclose(d_s[4], d_sc[1].double() / ncrops, rtol=1e-12, atol=0)
    d_f2, d_s2 = ref.magnitude_bwd(f, d_mag, None, bs, ncrops)
    assert torch.equal(d_f2, d_f) and not d_s2.any()


@pytest.mark.parametrize("bs,T,ncrops,k,F", [(4, 32, 10, 3, 1024), (32, 32, 10, 3, 1024), (2, 5, 2, 2, 17)])
def test_float64_loss_agrees_with_the_float32_oracle(bs, T, ncrops, k, F):
    """The inputs and the tolerances of test_hip_mgfn.py::test_mgfn_loss_fwd_bwd_vs_oracle."""
    from oracle import mgfn_oracle

    n = bs // 2
    sc = synth_tensor(f"k10.sc.{bs}", (bs, T, 1), scale=0.45, offset=0.5)
    sa = synth_tensor(f"k10.sa.{bs}", (n, 1), scale=0.4, offset=0.5)
    sn = synth_tensor(f"k10.sn.{bs}", (n, 1), scale=0.4, offset=0.5)
    fa = synth_tensor(f"k10.fa.{bs}", (ncrops * n, k, F), scale=1.0, offset=0.05)
    fn = synth_tensor(f"k10.fn.{bs}", (ncrops * n, k, F), scale=0.8)
    al, nl = torch.ones(n), torch.zeros(n)
    cpu = [t.clone().requires_grad_(True) for t in (sc, sa, sn, fa, fn)]
    l_mgfn, terms = mgfn_oracle.mgfn_loss(cpu[1], cpu[2], cpu[3], cpu[4], al, nl)
    smooth = mgfn_oracle.smoothness_loss(cpu[0])
    sparse = mgfn_oracle.sparsity_loss(cpu[0][: bs // 2].reshape(-1))
    total = l_mgfn + smooth + sparse
    (total * 1.7).backward()
    t64, g64 = ref.loss(sc, sa, sn, fa, fn, al, nl, g=1.7)
    got = dict(total=total, bce=terms["cls"], con=terms["con"], con_a=terms["con_a"], con_n=terms["con_n"], smooth=smooth, sparse=sparse,
               mgfn=l_mgfn)
    assert tuple(t64) == ref.LOSS_TERMS
    for name in ref.LOSS_TERMS:
        assert rel_err(got[name].detach(), t64[name]) < 1e-5, name
    for a, b, name in zip(cpu, g64, ("scores", "abn", "nor", "a_feat", "n_feat")):
        assert b.dtype == torch.float64 and b.shape == a.shape
        assert rel_err(a.grad, b) < 1e-4, name


def test_float64_bce_of_saturated_and_denormal_scores():
    p = np.array([0.0, 1.0, 1e-40, 1.0 - 2.0 ** -24], np.float32)
    val, gr = ref.bce(p, np.array([1.0, 0.0, 1.0, 1.0]))
    want = (100 + 100 - np.log(np.float64(np.float32(1e-40))) - np.log1p(-(2.0 ** -24))) / 4
    assert val == pytest.approx(want, rel=1e-12)
    assert -np.log(np.float64(np.float32(1e-40))) == pytest.approx(92.1034, rel=1e-5)  # not the clamp's 100
    assert gr[0].item() == pytest.approx(-1 / 1e-12 / 4) and gr[1].item() == pytest.approx(1 / 1e-12 / 4)
