"""The conv launchers' table of algorithm ids (csrc/conv_igemm.hip: ALGO_TABLE), seen through advhip_conv3d_algo_info.

Host: the table against a frozen literal and against _lib's *_ALGOS tuples; the split-K workspace sizes against a recording of the
revision before the table (tests/golden/conv_workspace_bytes.json, tools/gen_conv_workspace_golden.py).
GPU: every row launches the kernel it names -- a row bound to the wrong kernel, or to none, shows here.
"""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN, rel_err

# id -> (BM, BN, BK): _lib.algo_tile of the revision that still computed it in Python, over every id that revision accepted and the
# T-fold ids.  (Id 0, ADVHIP_ALGO_AUTO, is the one entry not taken from there: that arithmetic gave (64, 128, 16) for an id it was
# never asked about, where the launcher's own choice for AUTO is, and was, the 64 x 64 x 16 tile -- which the query reports.)
FROZEN_TILES = {
    0: (64, 64, 16), 1: (128, 128, 16), 2: (128, 64, 16), 3: (64, 64, 16), 4: (64, 128, 16), 5: (128, 128, 32), 6: (128, 64, 32),
    7: (64, 64, 32), 8: (64, 128, 32), 33: (128, 128, 16), 34: (128, 64, 16), 35: (64, 64, 16), 36: (64, 128, 16),
    37: (128, 128, 32), 38: (128, 64, 32), 39: (64, 64, 32), 40: (64, 128, 32), 65: (128, 128, 16), 66: (128, 64, 16),
    67: (64, 64, 16), 68: (64, 128, 16), 70: (128, 64, 32), 71: (64, 64, 32), 72: (64, 128, 32), 98: (128, 64, 16), 99: (64, 64, 16),
    100: (64, 128, 16), 133: (128, 128, 32), 134: (128, 64, 32), 161: (128, 128, 16), 162: (128, 64, 16), 163: (64, 64, 16),
    164: (64, 128, 16), 166: (128, 64, 32), 167: (64, 64, 32), 168: (64, 128, 32), 169: (256, 64, 16), 192: (128, 64, 16),
    200: (128, 64, 16), 209: (128, 128, 16), 210: (128, 64, 16), 211: (64, 64, 16), 212: (64, 128, 16), 214: (128, 64, 32),
    215: (64, 64, 32), 216: (64, 128, 32), 217: (256, 64, 16), 226: (128, 64, 16), 227: (64, 64, 16), 234: (128, 64, 16),
    235: (64, 64, 16), 242: (128, 64, 16), 243: (64, 64, 16),
}


def _query(lib, algo):
    out = [C.c_int32(-7) for _ in range(4)]
    rc = lib.advhip_conv3d_algo_info(algo, *(C.byref(o) for o in out))
    return rc, tuple(o.value for o in out)


def _accepted():
    """{id: (family name, BM, BN, BK)} of every id in [0, 300) the query accepts"""
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    return {a: _lib.algo_info(a) for a in range(300) if _query(lib, a)[0] == 0}


def test_algo_table_matches_frozen_literal_and_lib_tuples():
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    for algo in range(0, 300):
        rc, (fam, bm, bn, bk) = _query(lib, algo)
        if algo in FROZEN_TILES:
            assert rc == 0 and (bm, bn, bk) == FROZEN_TILES[algo], (algo, rc, (bm, bn, bk), lib.advhip_last_error())
            assert 0 <= fam < len(_lib.FAMILIES), (algo, fam)
            assert _lib.algo_tile(algo) == FROZEN_TILES[algo]
        else:
            assert rc == -1 and (fam, bm, bn, bk) == (-7, -7, -7, -7), (algo, rc)
            assert b"not instantiated" in lib.advhip_last_error(), (algo, lib.advhip_last_error())
    assert lib.advhip_conv3d_algo_info(3, None, None, None, None) == 0  # every output is optional
    # a literal in _lib.py without a row, or a row without its literal
    listed = (set(_lib.IGEMM_ALGOS) | set(_lib.FAST_ALGOS) | set(_lib.DMA_ALGOS) | set(_lib.DMA4_ALGOS) | set(_lib.BF16X3_ALGOS) | set(_lib.DMA2_ALGOS)
              | set(_lib.PERSIST_ALGOS) | {0, _lib.ALGO_TSPAN_128x64, _lib.ALGO_MIXED_128x64})
    accepted = set(_accepted())
    tfold = {a for a in accepted if _lib.is_tfold(a)}
    assert tfold == set(_lib.TFOLD_ALGOS)
    assert accepted - tfold == listed, (sorted(listed - accepted), sorted(accepted - tfold - listed))
    # the family of an id is its tuple's; a T-fold id reports the 2-deep-ring kernel its folded launch runs
    fams = {"generic": _lib.IGEMM_ALGOS, "fast": _lib.FAST_ALGOS, "dma3": _lib.DMA_ALGOS + (0,), "dma4": _lib.DMA4_ALGOS, "bf16x3": _lib.BF16X3_ALGOS,
            "dma2": _lib.DMA2_ALGOS + _lib.TFOLD_ALGOS, "tspan": (_lib.ALGO_TSPAN_128x64,), "mixed": (_lib.ALGO_MIXED_128x64,), "persist": _lib.PERSIST_ALGOS}
    assert set(fams) == set(_lib.FAMILIES)
    for fam, ids in fams.items():
        for a in ids:
            assert _lib.algo_info(a)[0] == fam, (a, fam, _lib.algo_info(a))
    with pytest.raises(_lib.HipExtensionError, match="not instantiated"):
        _lib.algo_tile(69)


def test_conv_workspace_bytes_unchanged():
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    rows = json.load(open(os.path.join(GOLDEN, "conv_workspace_bytes.json")))
    assert len(rows) == 3 * 13 * 3 + 3 and len({(tuple(r["desc"]), r["algo"], r["splits"]) for r in rows}) == len(rows)
    assert sum(r["bytes"] > 0 for r in rows) >= 70 and sum(r["bytes"] == -1 for r in rows) == 3
    for r in rows:
        b, cin, t, h, w, cout, kt, kh, kw, pt, ph, pw = r["desc"]
        d = _lib.ConvDesc(b, cin, t, h, w, cout, kt, kh, kw, 1, 1, 1, pt, ph, pw, 1, r["algo"], r["splits"])
        assert lib.advhip_conv3d_workspace_bytes(C.byref(d)) == r["bytes"], r


# ---- GPU: every row launches the kernel it names ---------------------------------------------------------------------------------
# (name, kernel, padding, (B, T, H, W)), Cin = 64, Cout = 128, stride 1.  a: M = 1 144 -- a partial last tile for every BM, rows a
# multiple of 4, K = 64 (the persistent kernels' minimum); b: rows of 98 positions, the virtually padded path.  The temporal conv
# carries ADVHIP_ALGO_TSPAN and the T-fold ids; those need T <= pt + 1 = 2 frames, which only shape b has.
CASES = [("a.k1", (1, 1, 1), (0, 0, 0), (2, 4, 13, 11)), ("b.k1", (1, 1, 1), (0, 0, 0), (2, 2, 7, 7)),
         ("a.t3", (3, 1, 1), (1, 0, 0), (2, 4, 13, 11)), ("b.t3", (3, 1, 1), (1, 0, 0), (2, 2, 7, 7))]
CIN, COUT = 64, 128


def _excluded(algo, info, k, t):
    """The documented precondition of `algo` that a (k, stride 1) conv on t frames to COUT channels does not meet, or None"""
    from anomaly_detection_on_video_amd import _lib

    fam, bm, bn, bk = info
    if COUT % bn:
        return "Cout not a multiple of the N tile"
    if _lib.is_tfold(algo):
        return None if (k[0] > 1 and t <= k[0] // 2 + 1) else "the T-fold takes (kt,1,1) convs on T <= kt/2 + 1 frames"
    if (fam == "tspan") != (k[0] > 1):
        return "TSPAN is for (kt,1,1) temporal convs (and the temporal cases are here for it and the T-fold alone)"
    return None


@pytest.mark.gpu
def test_every_algo_row_launches_its_kernel():
    from anomaly_detection_on_video_amd import _lib, ops
    from anomaly_detection_on_video_amd.weights import synth_tensor
    from oracle import i3d_oracle
    from test_hip_i3d import BF16X3_TOL, TIGHT

    dev = torch.device("cuda:0")
    accepted = _accepted()
    assert set(accepted) == set(FROZEN_TILES)
    dma2_of_tile = {info[1:]: a for a, info in accepted.items() if info[0] == "dma2" and not _lib.is_tfold(a)}
    ran = {name: set() for name, *_ in CASES}
    bad = []
    for name, k, p, bthw in CASES:
        b, t, h, w = bthw
        x = synth_tensor(f"algotab.{name}.x", (b, CIN, t, h, w), scale=2.0)
        wt = synth_tensor(f"algotab.{name}.w", (COUT, CIN) + k, scale=float((6.0 / (CIN * k[0])) ** 0.5))
        g, be = synth_tensor(f"algotab.{name}.g", (COUT,), scale=0.5, offset=1.0), synth_tensor(f"algotab.{name}.b", (COUT,), scale=0.25)
        mu, var = synth_tensor(f"algotab.{name}.m", (COUT,), scale=0.25), synth_tensor(f"algotab.{name}.v", (COUT,), scale=0.5, offset=1.0)
        ref = i3d_oracle.conv_bn_act(x, wt, g, be, mu, var, (1, 1, 1), p, None, True)
        pc = ops.pack_conv(wt.to(dev), g.to(dev), be.to(dev), mu.to(dev), var.to(dev), 1e-5, (1, 1, 1), p, name=f"algotab.{name}")
        xd = x.to(dev)
        outs = {}
        for algo, info in sorted(accepted.items()):
            if _excluded(algo, info, k, t) is not None:
                continue
            out = torch.full(tuple(ref.shape), float("nan"), device=dev)
            got = ops.conv3d_bn_act(xd, pc, relu=True, algo=algo, splits=1, out=out)
            assert got.data_ptr() == out.data_ptr()
            outs[algo] = out
            ran[name].add(algo)
            e = rel_err(out.cpu(), ref)  # (NaN left anywhere: e is NaN and the comparison below fails)
            tol = BF16X3_TOL if info[0] == "bf16x3" else TIGHT
            if not e < tol:
                bad.append(f"{name} algo {algo} {info}: rel err {e:.3e} (bound {tol:.0e})")
        # the families DESIGN.md documents as bit-identical to the plain 2-deep-ring kernel of the same tile
        for algo, out in outs.items():
            if accepted[algo][0] in ("mixed", "persist") and not torch.equal(out, outs[dma2_of_tile[accepted[algo][1:]]]):
                bad.append(f"{name} algo {algo}: differs from algo {dma2_of_tile[accepted[algo][1:]]}")
    assert not bad, "\n".join(bad)
    # nothing is left out but what the preconditions exclude: every id of every family but TSPAN runs on both 1x1x1 cases, TSPAN on
    # both temporal ones, the T-fold ids where T allows them -- and on shape a every family runs
    plain = {a for a, info in accepted.items() if not _lib.is_tfold(a) and info[0] != "tspan"}
    assert ran["a.k1"] == plain and ran["b.k1"] == plain
    assert ran["a.t3"] == {_lib.ALGO_TSPAN_128x64} and ran["b.t3"] == {_lib.ALGO_TSPAN_128x64} | set(_lib.TFOLD_ALGOS)
    assert {accepted[a][0] for a in ran["a.k1"] | ran["a.t3"]} == set(_lib.FAMILIES)
