"""GPU tests of the five GlanceAttention kernels (csrc/mgfn.hip: glance_attn_fwd / _bwd at T = 32, glance_attn_fwd_anyt<LENS> below
256 clips, glance_attn_fwd_mfma<LENS> from 256 on, glance_attn_bwd_anyt) at their tile edges, against independent truth
(tests/_attention_ref.py; tests/test_attention_ref_host.py checks that truth without a GPU).

Technique, as in tests/test_hip_scorer_forms.py: the C entry points are called on test-owned buffers.  Every input is a view inside a
NaN-filled buffer (64 floats on either side: a read past an end poisons the result), every output a view inside a sentinel-filled
one; after every launch the guard floats must keep their bits and every element the kernel owns must be written.  Every case runs
aligned and one float further in; these kernels use scalar global accesses, so both placements must give the same bits.

T edges: 32 (the one-tile kernels; the any-T entry point runs there too, as the `_lens` form of a 32-clip batch does); 1, 2, 31, 33, 63,
64, 65, 255 (32-key tiles, full or ragged tail); 256, 257, 271, 272, 319, 320, 321 (64 x 64 tiles of the matrix pipe, a wave's 16 queries
partly or just filled, tails of 0, 1, 15, 16, 63, 0, 1 clips).  Exact cases (one-hot codes, uniform weights) are compared with `==`;
random data against fp64 at the project's 1e-5 per (sequence, head) slice; peaked softmax at max(1e-5, 4 e_cpu) per tensor, e_cpu
being what fp32 torch on the CPU loses on the same inputs; non-finite inputs against the fp64 reference's NaN mask, with every other
(sequence, head) keeping the bits of the clean launch."""
import ctypes as C
import functools

import pytest
import torch

from conftest import rel_err
import _attention_ref as ref
from test_hip_scorer_forms import DEV, Buf, Out

pytestmark = pytest.mark.gpu
SCALE = ref.SCALE
BOUND = 1e-5  # the bound of tests/test_hip_mgfn.py for the same op
DH = ref.D
PLACEMENTS = (("aligned", False), ("one float in", True))


def _m():
    from anomaly_detection_on_video_amd import _lib

    return _lib


def _after_launch(inputs, outputs):
    for name, b in list(inputs.items()) + list(outputs.items()):
        assert b.guards_intact(), f"the guard floats around {name} changed"
    for name, b in outputs.items():
        assert b.all_written(), f"{name} still holds sentinel values"


def kernels_at(T):
    return ("tile", "anyt") if T == 32 else ("anyt",)


def fwd_tile(qkv, heads, B, T, mis):
    m = _m()
    x, out, p = Buf(qkv, mis), Out((heads * DH, B, T), mis), Out((B, heads, T, T), mis)
    m.check(m.load().advhip_glance_attention_fwd_f32(x.p, out.p, p.p, heads, B, T, DH, C.c_float(SCALE), m.stream(x.t)), "glance_attention_fwd")
    _after_launch({"qkv": x}, {"out": out, "p": p})
    return out.t, p.t


def fwd_anyt(qkv, heads, B, T, mis, want_lse=True):
    m = _m()
    x, out = Buf(qkv, mis), Out((heads * DH, B, T), mis)
    lse = Out((B, heads, T), mis) if want_lse else None
    m.check(m.load().advhip_glance_attention_fwd_anyt_f32(x.p, out.p, lse.p if want_lse else None, heads, B, T, DH, C.c_float(SCALE), m.stream(x.t)),
            "glance_attention_fwd_anyt")
    _after_launch({"qkv": x}, {"out": out, "lse": lse} if want_lse else {"out": out})
    return out.t, (lse.t if want_lse else None)


def fwd_lens(qkv, lens, heads, B, T, mis):
    m = _m()
    x, out = Buf(qkv, mis), Out((heads * DH, B, T), mis)
    raw = torch.full((B + 128,), 1 << 30, dtype=torch.int32, device=DEV)  # a length read past either end is a huge one
    raw[64:64 + B] = torch.as_tensor(lens, dtype=torch.int32)
    m.check(m.load().advhip_glance_attention_fwd_lens_f32(x.p, out.p, raw[64:64 + B].data_ptr(), heads, B, T, DH, C.c_float(SCALE), m.stream(x.t)),
            "glance_attention_fwd_lens")
    _after_launch({"qkv": x}, {"out": out})
    return out.t


def bwd_tile(dout, qkv, p, heads, B, T, mis):
    m = _m()
    g, x, pb, dqkv = Buf(dout, mis), Buf(qkv, mis), Buf(p, mis), Out((3 * heads * DH, B, T), mis)
    m.check(m.load().advhip_glance_attention_bwd_f32(g.p, x.p, pb.p, dqkv.p, heads, B, T, DH, C.c_float(SCALE), m.stream(x.t)), "glance_attention_bwd")
    _after_launch({"dout": g, "qkv": x, "p": pb}, {"dqkv": dqkv})
    return dqkv.t


def bwd_anyt(dout, qkv, out, lse, heads, B, T, mis):
    m = _m()
    g, x, ob, lb, dqkv = Buf(dout, mis), Buf(qkv, mis), Buf(out, mis), Buf(lse, mis), Out((3 * heads * DH, B, T), mis)
    m.check(m.load().advhip_glance_attention_bwd_anyt_f32(g.p, x.p, ob.p, lb.p, dqkv.p, heads, B, T, DH, C.c_float(SCALE), m.stream(x.t)),
            "glance_attention_bwd_anyt")
    _after_launch({"dout": g, "qkv": x, "out": ob, "lse": lb}, {"dqkv": dqkv})
    return dqkv.t


def run(kernel, qkv, dout, heads, B, T, mis):
    """Forward and backward through one kernel family: -> dict(out, p | lse, dq, dk, dv).  The backward is fed what the forward wrote."""
    inner = heads * DH
    if kernel == "tile":
        out, p = fwd_tile(qkv, heads, B, T, mis)
        res = {"out": out, "p": p}
        dqkv = bwd_tile(dout, qkv, p, heads, B, T, mis)
    else:
        out, lse = fwd_anyt(qkv, heads, B, T, mis)
        res = {"out": out, "lse": lse}
        dqkv = bwd_anyt(dout, qkv, out, lse, heads, B, T, mis)
    res.update(dq=dqkv[:inner], dk=dqkv[inner:2 * inner], dv=dqkv[2 * inner:])
    return res


def run_both_placements(kernel, qkv, dout, heads, B, T):
    """The aligned result, after asserting that the other placement gives the same bits."""
    res = run(kernel, qkv, dout, heads, B, T, False)
    other = run(kernel, qkv, dout, heads, B, T, True)
    for name, t in res.items():
        assert ref.same_bits(t, other[name]), f"{kernel} T={T}: {name} differs between the two placements"
    return res


def _pair_name(pair, heads):
    return f"(b={pair // heads}, h={pair % heads})"


# ---- the one-hot construction -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mapping", ref.MAPPINGS)
@pytest.mark.parametrize("T", ref.T_EDGES)
def test_one_hot_forward_is_the_gather_bit_for_bit(T, mapping):
    """Every key counted once, in the right query's row: out[:, b, i] = v[:, b, mapping(i)] with the bits of v (arbitrary fp32), lse =
    128 nb exactly, p exactly one-hot at T = 32; the launch without lse gives the same out."""
    heads, B = ref.geometry(T)
    case = ref.one_hot_case(heads, B, T, mapping, seed=T)
    want = case["out"].to(DEV)
    for place, mis in PLACEMENTS:
        if T == 32:
            out, p = fwd_tile(case["qkv"], heads, B, T, mis)
            assert ref.same_bits(out, want), ("tile", place)
            assert torch.equal(p, torch.nn.functional.one_hot(case["idx"], T).float().to(DEV)), ("tile", place)
        out, lse = fwd_anyt(case["qkv"], heads, B, T, mis)
        assert ref.same_bits(out, want), place
        assert bool((lse == case["lse"]).all()), (place, lse.flatten()[:4].tolist(), case["lse"])
        out_only, _ = fwd_anyt(case["qkv"], heads, B, T, mis, want_lse=False)
        assert ref.same_bits(out_only, want), (place, "no lse")


@pytest.mark.parametrize("mapping", ref.MAPPINGS)
@pytest.mark.parametrize("T", ref.T_EDGES)
def test_one_hot_backward_is_the_scatter_sum_and_zero(T, mapping):
    """Integer v and dout: dv = the scatter-sum of dout exactly, dq = dk = 0 (compared with ==: -0.0 passes).  T = 32 through the
    one-tile pair (p must come out exactly one-hot), every T through the any-T pair: out and lse from the vector forward below 256
    clips and from the matrix-pipe forward from there on."""
    heads, B = ref.geometry(T)
    case = ref.one_hot_case(heads, B, T, mapping, seed=T, integer=True)
    want_dv = case["dv"].to(DEV)
    for kernel in kernels_at(T):
        res = run_both_placements(kernel, case["qkv"], case["dout"], heads, B, T)
        assert torch.equal(res["out"], case["out"].to(DEV)), kernel
        if kernel == "tile":
            assert torch.equal(res["p"], torch.nn.functional.one_hot(case["idx"], T).float().to(DEV))
        else:
            assert bool((res["lse"] == case["lse"]).all())
        assert torch.equal(res["dv"], want_dv), kernel
        assert bool((res["dq"] == 0).all()) and bool((res["dk"] == 0).all()), kernel


@pytest.mark.parametrize("T,lens", [(40, (1, 31, 32, 33, 40)), (321, (1, 63, 64, 65, 256, 257, 321))], ids=["T40", "T321"])
def test_one_hot_with_lengths(T, lens):
    """advhip_glance_attention_fwd_lens_f32 against truth instead of against the un-padded launch: each row's codes are built for its
    own length, NaN sits behind its end; out[:, r, :L] is the gather bit for bit and out[:, r, L:] is 0."""
    heads, B = 2, len(lens)
    case = ref.one_hot_lens_case(heads, T, lens, seed=T)
    want = case["out"].to(DEV)
    for place, mis in PLACEMENTS:
        out = fwd_lens(case["qkv"], lens, heads, B, T, mis)
        for r, L in enumerate(lens):
            assert ref.same_bits(out[:, r, :L], want[:, r, :L]), (place, r, L)
            assert not bool(out[:, r, L:].any()), (place, r, L)


# ---- the uniform construction ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", ref.T_EDGES)
def test_uniform_forward_is_the_mean(T):
    """q = 0: every key weighs 1, l = T.  out within 2^-23 |mean| of the exact mean, exactly the mean at a power of two or a zero sum;
    lse = log T (exactly 0 at T = 1).  A key dropped, a zero-filled key counted or a tile counted twice changes l."""
    heads, B = ref.geometry(T)
    case = ref.uniform_case(heads, B, T, seed=T)
    worst = 0.0
    for place, mis in PLACEMENTS:
        if T == 32:
            out, p = fwd_tile(case["qkv"], heads, B, T, mis)
            ref.check_uniform(case, out)
            assert bool((p == 1.0 / 32).all())
        out, lse = fwd_anyt(case["qkv"], heads, B, T, mis)
        worst = max(worst, ref.check_uniform(case, out, lse))
    print(f"uniform T={T}: worst |out - mean| = {worst:.3f} x 2^-23 |mean|")


# ---- the chunk loop of the launchers --------------------------------------------------------------------------------------------

def _pairs_that_differ(got, want, heads):
    bad = (ref.per_pair(got, heads) != ref.per_pair(want, heads)).any(dim=1).nonzero().flatten()
    if bad.numel() == 0:
        return None
    return f"{bad.numel()} (sequence, head) pairs differ, first {_pair_name(int(bad[0]), heads)}, last {_pair_name(int(bad[-1]), heads)}"


def test_chunk_loop_of_the_any_t_launchers():
    """heads = 3, B = 10 924: 32 772 (sequence, head) pairs, four of them in the launchers' second grid (bh0 = 32 768), at T = 2.
    One-hot case with a seeded mapping per pair, integer v and dout; the expected gather / scatter by torch indexing on the device.
    advhip_glance_attention_fwd_anyt_f32, _fwd_lens_f32 (lengths alternating 1 and 2, NaN behind the ends) and _bwd_anyt_f32 must be
    exact over the whole tensor.  (Not here: the matrix-pipe kernel beyond 32 768 pairs -- 6 GB of operands at T = 256; its bh0
    arithmetic is the same two lines.)"""
    heads, B, T = 3, 10924, 2
    assert B * heads == 32768 + 4
    inner = heads * DH
    gen = torch.Generator().manual_seed(20)
    idx = torch.randint(0, T, (B, heads, T), generator=gen).to(DEV)
    v = torch.randint(-8, 9, (inner, B, T), generator=gen).float().to(DEV)
    dout = torch.randint(-8, 9, (inner, B, T), generator=gen).float().to(DEV)
    qkv = ref.one_hot_qkv(idx, v)
    assert qkv.device.type == "cuda" and qkv.numel() * 4 > 50e6
    want = ref.gather_v(v, idx)
    out, lse = fwd_anyt(qkv, heads, B, T, False)
    assert _pairs_that_differ(out, want, heads) is None, "fwd_anyt: " + _pairs_that_differ(out, want, heads)
    assert bool((lse == 128.0).all()), "fwd_anyt lse: " + str(_pairs_that_differ(lse, torch.full_like(lse, 128.0), heads))
    dqkv = bwd_anyt(dout, qkv, out, lse, heads, B, T, False)
    want_dv = ref.scatter_dout(dout, idx)
    assert _pairs_that_differ(dqkv[2 * inner:], want_dv, heads) is None, "bwd_anyt dv: " + _pairs_that_differ(dqkv[2 * inner:], want_dv, heads)
    zero = torch.zeros_like(want)
    for name, part in (("dq", dqkv[:inner]), ("dk", dqkv[inner:2 * inner])):
        assert _pairs_that_differ(part, zero, heads) is None, f"bwd_anyt {name}: " + _pairs_that_differ(part, zero, heads)
    del dqkv, lse, out
    lens = torch.ones(B, dtype=torch.int32)
    lens[1::2] = 2
    padded = qkv.clone()
    padded[:, 0::2, 1] = float("nan")  # behind the end of the one-clip rows
    want_lens = want.clone()
    want_lens[:, 0::2, 0] = v[:, 0::2, 0]  # one key: it takes all the weight whatever the query says
    want_lens[:, 0::2, 1] = 0
    got = fwd_lens(padded, lens, heads, B, T, False)
    assert _pairs_that_differ(got, want_lens, heads) is None, "fwd_lens: " + _pairs_that_differ(got, want_lens, heads)


# ---- random data against fp64 ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_reference(T):
    heads, B = ref.geometry(T)
    qkv, dout = ref.random_inputs(heads, B, T)
    return qkv, dout, ref.attention_fp64(qkv, heads, SCALE, dout)


def _slice_report(head, res, want, heads, names, bound=BOUND):
    items = []
    for name in names:
        err, pair = ref.slice_errors(res[name], want[name], heads)
        items.append((name, err, pair))
    print(f"{head}: " + ", ".join(f"{n} {e:.2e} at {_pair_name(p, heads)}" for n, e, p in items))
    bad = [(n, e, _pair_name(p, heads)) for n, e, p in items if not e < bound]
    assert not bad, (head, bad)


@pytest.mark.parametrize("T", ref.T_EDGES)
def test_random_data_vs_fp64_per_sequence_and_head(T):
    """Scale-1.5 inputs, forward and backward, against fp64 autograd at rel_err < 1e-5 taken over each (sequence, head) slice on its
    own, for out, lse (p at T = 32), dq, dk and dv separately; two launches and the two placements give equal bits."""
    heads, B = ref.geometry(T)
    qkv, dout, want = _random_reference(T)
    for kernel in kernels_at(T):
        res = run_both_placements(kernel, qkv, dout, heads, B, T)
        again = run(kernel, qkv, dout, heads, B, T, False)
        for name, t in res.items():
            assert ref.same_bits(t, again[name]), f"{kernel} T={T}: {name} differs between two launches"
        _slice_report(f"random {kernel} heads={heads} B={B} T={T}", res, want, heads, ("out", "p" if kernel == "tile" else "lse", "dq", "dk", "dv"))


# ---- peaked softmax -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads,B,T", ref.PEAKED_SHAPES, ids=[f"T{t}" for _, _, t in ref.PEAKED_SHAPES])
def test_peaked_softmax_forward_and_backward(heads, B, T):
    """Scale-6.0 inputs (|logit| up to ~60, the top key holds most of a row's weight): T = 32 through the one-tile pair, T = 100
    through the vector forward, T = 333 through the matrix-pipe forward, whose lse the any-T backward re-derives p from with logits
    summed in another order.  Bound per tensor: max(1e-5, 4 e_cpu), e_cpu = rel_err of fp32 torch autograd on the CPU against fp64 on
    the same inputs; the factor 4 covers a logit of magnitude ~60 rounded twice (forward and backward orders) and one rescale per key
    tile.  Measured (MI355X): see DESIGN.md section 7."""
    qkv, dout = ref.peaked_inputs(heads, B, T)
    want = ref.attention_fp64(qkv, heads, SCALE, dout)
    e_cpu = ref.cpu_fp32_yardstick(qkv, dout, heads, want)
    kernel = "tile" if T == 32 else "anyt"
    res = run_both_placements(kernel, qkv, dout, heads, B, T)
    assert all(bool(torch.isfinite(t).all()) for t in res.values())
    errs = {name: rel_err(res[name].cpu(), want[name]) for name in ("out", "dq", "dk", "dv")}
    bounds = {name: max(BOUND, 4 * e_cpu[name]) for name in errs}
    print(f"peaked {kernel} heads={heads} B={B} T={T}: " + ", ".join(f"{n} e_cpu {e_cpu[n]:.2e} kernel {errs[n]:.2e} bound {bounds[n]:.2e}" for n in errs))
    bad = {n: (errs[n], bounds[n]) for n in errs if not errs[n] < bounds[n]}
    assert not bad, bad


# ---- non-finite inputs --------------------------------------------------------------------------------------------------------------

NF_HEADS, NF_B = 2, 2


@functools.lru_cache(maxsize=None)
def _clean_launch(kernel, T, positive_q):
    qkv, dout, _bq, _bd, _pair = ref.poison_case("k_neginf_column" if positive_q else "q_nan", NF_HEADS, NF_B, T, "first")
    return run_both_placements(kernel, qkv, dout, NF_HEADS, NF_B, T)


@pytest.mark.parametrize("where", ["first", "tail"])
@pytest.mark.parametrize("kind", ref.POISONS)
@pytest.mark.parametrize("T", [32, 40, 300])
def test_non_finite_inputs_come_out_where_torch_puts_them(T, kind, where):
    """One NaN / Inf in q, k, v or dout of the last (sequence, head), in the first tile or in the tail tile.  The NaN mask of every
    output equals the fp64 reference's (tests/test_attention_ref_host.py derives each by hand), the finite elements hold the
    random-data bound, nothing is Inf, and every other (sequence, head) has the bits of the clean launch.
      NaN in q[d, b, i]     query i: out, lse, dq are NaN (every channel); dk and dv of the pair are NaN
      NaN in k[d, b, j]     the whole pair is NaN (the row maxima go through fmaxf, which drops the NaN: exp and the sums carry it)
      NaN in v[d, b, j]     out[d, b, :] is NaN and nothing else of out; dq, dk of the pair are NaN, dv is clean
      +Inf in k[d, b, j]    queries with q[d] > 0 are NaN (Inf - Inf); those with q[d] < 0 give key j weight 0 and stay finite but
                            for dq[d] (0 * Inf)
      -Inf in k, q[d] > 0   a whole key column of weight 0: everything finite but dq[d, b, :] (0 * Inf)
      NaN in dout[d, b, i]  dq[:, b, i], dk of the pair and dv[d, b, :] are NaN; the forward is untouched"""
    heads, B = NF_HEADS, NF_B
    qkv, dout, bad_qkv, bad_dout, (pb, ph) = ref.poison_case(kind, heads, B, T, where)
    want = ref.nonfinite_expectation(bad_qkv, bad_dout, heads)
    others = torch.arange(B * heads) != pb * heads + ph
    for kernel in kernels_at(T):
        clean = _clean_launch(kernel, T, kind == "k_neginf_column")
        res = run_both_placements(kernel, bad_qkv, bad_dout, heads, B, T)
        names = ("out", "p" if kernel == "tile" else "lse", "dq", "dk", "dv")
        for name in names:
            got = res[name].cpu()
            assert torch.equal(torch.isnan(got), want[name][1]), (kernel, name, int(torch.isnan(got).sum()), int(want[name][1].sum()))
            assert not bool(torch.isinf(got).any()), (kernel, name)
            assert ref.same_bits(ref.per_pair(got, heads)[others], ref.per_pair(clean[name].cpu(), heads)[others]), \
                f"{kernel} {name}: a (sequence, head) other than the poisoned one changed"
        _slice_report(f"{kind} {where} {kernel} T={T}", res, {n: want[n][0] for n in names}, heads, names)
