"""Plain references of the MIL head and loss kernels (csrc/mil.hip, csrc/loss.hip) for tests/test_hip_mil_edges.py and
tests/test_mil_ref_host.py.  numpy / CPU torch only, float64 unless a line says otherwise; nothing here calls the package.

The order of the top-k is the kernel's documented one ("MIL top-k order"): NaN first, then the larger value, then the
lower index.  `torch.topk` on the CPU is NOT a reference for it: it breaks ties in no stated order."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mgfn_oracle

LOSS_TERMS = ("total", "bce", "con", "con_a", "con_n", "smooth", "sparse", "mgfn")


def _np(t, dtype):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=dtype)


def topk_order(values_f32, k):
    """(n, T) or (T,) fp32 -> int64 (n, k) or (k,): the first k indices by the key (is-NaN first, larger value first, lower index
    first).  +0 and -0 compare equal; -inf is an ordinary smallest value."""
    v = _np(values_f32, np.float32)
    one = v.ndim == 1
    v = np.atleast_2d(v)
    out = np.empty((v.shape[0], k), dtype=np.int64)
    index = np.arange(v.shape[1])
    for r, row in enumerate(v):
        nan = np.isnan(row)
        neg = -np.where(nan, np.float32(0), row).astype(np.float64)  # ascending -value = descending value; -0.0 == 0.0
        # lexsort: the LAST key is the primary one
        out[r] = np.lexsort((index, neg, ~nan))[:k]
    return out[0] if one else out


def select(features, scores, mag, keep, ncrops, k):
    """mil_topk_select.  features (n * ncrops, T, F) fp32, scores = the crop-mean scores (n, T), mag (n, T), keep (n, T) or None.
    -> idx (n, k) int64, sel (ncrops * n, k, F) fp32 (a copy of bits, crop-major), score (n,) float64."""
    feats = _np(features, np.float32)
    sc = _np(scores, np.float64)
    values = _np(mag, np.float32)
    if keep is not None:
        with np.errstate(invalid="ignore"):  # inf * 0 = NaN is one of the cases
            values = values * _np(keep, np.float32)  # ONE fp32 multiply: the kernel's bits
    n, T = values.shape
    idx = topk_order(values, k)
    fe = feats.reshape(n, ncrops, T, feats.shape[-1])
    sel = np.empty((ncrops * n, k, feats.shape[-1]), dtype=np.float32)
    for c in range(ncrops):
        for v in range(n):
            sel[c * n + v] = fe[v, c, idx[v]]
    score = np.take_along_axis(sc, idx, axis=1).mean(axis=1)
    return idx, sel, score


def select_bwd(idx, d_sel, d_score, shapes):
    """shapes = (n, ncrops, T, F, k).  -> d_features (n * ncrops, T, F) fp32: d_sel copied into zeros; d_sc (n, T) fp32:
    d_score[v] / k (one fp32 division) at the chosen positions, zero elsewhere."""
    n, ncrops, T, Fdim, k = shapes
    idx = _np(idx, np.int64)
    d_sel = _np(d_sel, np.float32)
    d_score = _np(d_score, np.float32).reshape(n)
    d_feat = np.zeros((n, ncrops, T, Fdim), dtype=np.float32)
    d_sc = np.zeros((n, T), dtype=np.float32)
    for v in range(n):
        assert len(set(idx[v].tolist())) == k, "the indices of one video must be distinct"
        for c in range(ncrops):
            d_feat[v, c, idx[v]] = d_sel[c * n + v]
        d_sc[v, idx[v]] = d_score[v] / np.float32(k)
    return d_feat.reshape(n * ncrops, T, Fdim), d_sc


def magnitude(features, scores, bs, ncrops):
    """-> mag (bs, T), sc (bs, T) in float64: the crop means of the rows' L2 norms and of the scores."""
    f = torch.as_tensor(_np(features, np.float64))
    s = torch.as_tensor(_np(scores, np.float64))
    T = f.shape[1]
    mag = torch.norm(f, p=2, dim=2).view(bs, ncrops, T).mean(1)
    sc = s.reshape(bs, ncrops, T).mean(1)
    return mag, sc


def magnitude_bwd(features, d_mag, d_sc, bs, ncrops):
    """float64 autograd of `magnitude`: -> d_features (bs * ncrops, T, F), d_scores (bs * ncrops, T).  `d_mag` / `d_sc` None: that
    output has no gradient.  The gradient of an all-zero row is zero (torch's subgradient of the norm at 0)."""
    f = torch.as_tensor(_np(features, np.float64)).requires_grad_(True)
    T = f.shape[1]
    s = torch.zeros((bs * ncrops, T), dtype=torch.float64, requires_grad=True)
    mag = torch.norm(f, p=2, dim=2).view(bs, ncrops, T).mean(1)
    sc = s.view(bs, ncrops, T).mean(1)
    obj = f.sum() * 0 + s.sum() * 0
    if d_mag is not None:
        obj = obj + (mag * torch.as_tensor(_np(d_mag, np.float64))).sum()
    if d_sc is not None:
        obj = obj + (sc * torch.as_tensor(_np(d_sc, np.float64))).sum()
    obj.backward()
    return f.grad, s.grad


def loss(scores, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels, g=1.0):
    """The float64 MGFN loss on the oracle's own functions.  scores (bs, T) or (bs, T, 1); abn / nor scores (n,) or (n, 1).
    -> (terms: dict over LOSS_TERMS of floats, grads: the gradients of g * total with respect to
    (scores, abn_score, nor_score, a_feat, n_feat), float64, in the inputs' shapes)."""
    ins = [torch.as_tensor(_np(t, np.float64)).requires_grad_(True) for t in (scores, abn_score, nor_score, a_feat, n_feat)]
    sc, sa, sn, fa, fn = ins
    al = torch.as_tensor(_np(abn_labels, np.float64))
    nl = torch.as_tensor(_np(nor_labels, np.float64))
    sc3 = sc if sc.dim() == 3 else sc.unsqueeze(2)
    bs = sc3.shape[0]
    l_mgfn, t = mgfn_oracle.mgfn_loss(sa.reshape(-1, 1), sn.reshape(-1, 1), fa, fn, al, nl)
    smooth = mgfn_oracle.smoothness_loss(sc3)
    sparse = mgfn_oracle.sparsity_loss(sc3[: bs // 2].reshape(-1))
    total = l_mgfn + smooth + sparse
    grads = torch.autograd.grad(total * g, ins, allow_unused=True)
    grads = [torch.zeros_like(i) if gr is None else gr for i, gr in zip(ins, grads)]
    terms = dict(total=total, bce=t["cls"], con=t["con"], con_a=t["con_a"], con_n=t["con_n"], smooth=smooth, sparse=sparse, mgfn=l_mgfn)
    return {name: float(terms[name].detach()) for name in LOSS_TERMS}, grads


def bce(p, y):
    """float64 `binary_cross_entropy` (mean) and its gradient with respect to p."""
    p = torch.as_tensor(_np(p, np.float64)).requires_grad_(True)
    out = F.binary_cross_entropy(p, torch.as_tensor(_np(y, np.float64)))
    (gr,) = torch.autograd.grad(out, p)
    return float(out.detach()), gr
