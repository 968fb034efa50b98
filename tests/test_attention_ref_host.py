"""CPU tests of tests/_attention_ref.py, the references and exact cases that tests/test_hip_attention_edges.py holds the
GlanceAttention kernels to: the builders produce what they claim in fp32 torch, in fp64 torch and under a tile-order fp32 emulation
of the online softmax (key tiles of 32 and of 64); every mutation of that emulation (a kernel bug restated) breaks an exact case;
the fp64 reference's NaN masks are the hand-derived ones; and the peaked-softmax yardstick e_cpu is printed."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
import _attention_ref as ref

HEADS, B = 2, 2
TILES = (32, 64)


def _all_pairs_lse(value, T):
    return torch.full((B, HEADS, T), float(value))


@pytest.mark.parametrize("T", ref.T_HOST)
def test_one_hot_case_is_the_gather_in_fp32_fp64_and_tile_order(T):
    for mapping in ref.MAPPINGS:
        case = ref.one_hot_case(HEADS, B, T, mapping, seed=T)
        qkv, want = case["qkv"], case["out"]
        assert case["lse"] == 128 * max(1, math.ceil(math.log2(T))) and qkv.shape == (3 * HEADS * 64, B, T)
        assert float(qkv[:2 * HEADS * 64].abs().max()) == 32.0
        assert 0 <= int(case["idx"].min()) and int(case["idx"].max()) < T
        r32 = ref.attention_torch(qkv, HEADS, ref.SCALE, dtype=torch.float32)
        assert ref.same_bits(r32["out"], want), (T, mapping)
        assert torch.equal(r32["lse"], _all_pairs_lse(case["lse"], T))
        assert torch.equal(r32["p"], torch.nn.functional.one_hot(case["idx"], T).float())
        r64 = ref.attention_fp64(qkv, HEADS, ref.SCALE)
        assert torch.equal(r64["out"], want.double()) and torch.equal(r64["lse"], _all_pairs_lse(case["lse"], T).double())
        for tile in TILES:
            em = ref.online_softmax_emulation(qkv, HEADS, ref.SCALE, tile)
            assert ref.same_bits(em["out"], want), (T, mapping, tile)
            assert torch.equal(em["lse"], _all_pairs_lse(case["lse"], T)) and not em["spill"]


def test_every_pair_sees_every_mapping():
    T = 33
    seen = {}
    for mapping in ref.MAPPINGS:
        idx = ref.pair_mappings(3, 2, T, mapping, seed=1).reshape(6, T)
        for pair in range(6):
            seen.setdefault(pair, set()).add(tuple(idx[pair].tolist()))
    assert all(len(s) == len(ref.MAPPINGS) for s in seen.values())
    idx = ref.pair_mappings(3, 2, T, "identity", seed=1)
    assert idx[0, 0].tolist() == list(range(T)) and idx[0, 1].tolist() == list(range(T - 1, -1, -1))
    assert sorted(idx[0, 2].tolist()) == list(range(T)) and idx[0, 2].tolist() != list(range(T))
    assert not idx[1, 0].any() and bool((idx[1, 1] == T - 1).all())


@pytest.mark.parametrize("T", ref.T_HOST)
def test_one_hot_backward_is_the_scatter_sum_and_zero(T):
    for mapping in ref.MAPPINGS:
        case = ref.one_hot_case(HEADS, B, T, mapping, seed=T, integer=True)
        v = case["qkv"][2 * HEADS * 64:]
        assert float(v.abs().max()) <= 8 and float(case["dout"].abs().max()) <= 8 and torch.equal(v, v.round())
        assert float(case["dv"].sum()) == float(case["dout"].sum())
        # the scatter against a plain loop
        b, h, d = B - 1, HEADS - 1, 7
        want = torch.zeros(T)
        for i in range(T):
            want[int(case["idx"][b, h, i])] += case["dout"][h * 64 + d, b, i]
        assert torch.equal(case["dv"][h * 64 + d, b], want)
        r32 = ref.attention_torch(case["qkv"], HEADS, ref.SCALE, case["dout"], torch.float32)
        assert torch.equal(r32["out"], case["out"]) and torch.equal(r32["dv"], case["dv"])
        assert bool((r32["dq"] == 0).all()) and bool((r32["dk"] == 0).all())
        # (fp64 keeps exp(-256) = 7e-112 where fp32 has 0: the same values to 1e-100)
        r64 = ref.attention_fp64(case["qkv"], HEADS, ref.SCALE, case["dout"])
        assert float((r64["dv"] - case["dv"].double()).abs().max()) < 1e-100
        assert float(r64["dq"].abs().max()) < 1e-100 and float(r64["dk"].abs().max()) < 1e-100


@pytest.mark.parametrize("T", ref.T_HOST)
def test_uniform_case_is_the_mean_within_its_bound(T):
    case = ref.uniform_case(HEADS, B, T, seed=T)
    qkv = case["qkv"]
    assert not qkv[:HEADS * 64].any() and case["mean"].shape == (HEADS * 64, B)
    assert torch.equal(case["vsum"], qkv[2 * HEADS * 64:].double().sum(dim=2))
    worst = 0.0
    # (torch normalises p = 1 / T before the second product, T roundings instead of one: held to the mean as floating point, and
    # exactly at the powers of two -- which is what the one-tile kernel, of the same formulation, is asked for at its T = 32)
    mean = case["mean"].unsqueeze(-1).expand(-1, -1, T)
    for dtype, bound in ((torch.float32, 1e-6), (torch.float64, 1e-14)):
        r = ref.attention_torch(qkv, HEADS, ref.SCALE, dtype=dtype)
        assert rel_err(r["out"], mean) < bound and rel_err(r["lse"], torch.full((B, HEADS, T), math.log(T), dtype=torch.float64)) < bound * 10
        if T & (T - 1) == 0:
            ref.check_uniform(case, r["out"], r["lse"])
    for tile in TILES:
        em = ref.online_softmax_emulation(qkv, HEADS, ref.SCALE, tile)
        worst = max(worst, ref.check_uniform(case, em["out"], em["lse"]))
    # the other way to divide, o * (1 / l) with its two roundings (o = the exact sum, as the accumulators hold it)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(T), dtype=torch.float32)
    worst = max(worst, ref.check_uniform(case, (case["vsum"].float() * inv).unsqueeze(-1).expand(-1, -1, T)))
    print(f"uniform T={T}: worst |out - mean| = {worst:.3f} x 2^-23 |mean|")
    assert worst <= 1.0


def test_check_uniform_refuses_a_wrong_count_and_a_wrong_lse():
    case = ref.uniform_case(1, 2, 33, seed=0)
    good = case["mean"].float().unsqueeze(-1).expand(-1, -1, 33)
    ref.check_uniform(case, good, torch.full((2, 1, 33), math.log(33)))
    with pytest.raises(AssertionError):
        ref.check_uniform(case, (case["vsum"] / 34).float().unsqueeze(-1).expand(-1, -1, 33))
    with pytest.raises(AssertionError):
        ref.check_uniform(case, good, torch.full((2, 1, 33), math.log(34)))
    with pytest.raises(AssertionError):
        ref.check_uniform(case, good * (1 + 3 * 2.0 ** -23))


def test_lens_case_rows_are_their_own_length_cases_with_nan_behind():
    lens = (1, 31, 32, 33, 40)
    case = ref.one_hot_lens_case(2, 40, lens, seed=3)
    for r, L in enumerate(lens):
        row = case["qkv"][:, r:r + 1, :L]
        assert not torch.isnan(row).any() and bool(torch.isnan(case["qkv"][:, r, L:]).all())
        got = ref.attention_torch(row, 2, ref.SCALE, dtype=torch.float32)
        assert ref.same_bits(got["out"], case["out"][:, r:r + 1, :L]) and bool((got["lse"] == 128 * ref.code_bits(L)).all())
        assert not case["out"][:, r, L:].any()


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_each_mutation_of_the_recurrence_breaks_an_exact_case(mutation):
    """A wrong kernel is caught: the mutated emulation loses bit equality with the gather (or the exact mean, or writes past the end
    of `out`) at the listed T.  Which T catch it is printed; the ones that must are asserted."""
    caught = {}
    for T in ref.T_HOST:
        for tile in TILES:
            hits = []
            for mapping in ref.MAPPINGS:
                case = ref.one_hot_case(HEADS, B, T, mapping, seed=T)
                em = ref.online_softmax_emulation(case["qkv"], HEADS, ref.SCALE, tile, mutation)
                if em["spill"] or not ref.same_bits(em["out"], case["out"]) or not bool((em["lse"] == case["lse"]).all()):
                    hits.append(mapping)
            case = ref.uniform_case(HEADS, B, T, seed=T)
            em = ref.online_softmax_emulation(case["qkv"], HEADS, ref.SCALE, tile, mutation)
            try:
                assert not em["spill"]
                ref.check_uniform(case, em["out"], em["lse"])
            except AssertionError:
                hits.append("uniform")
            if hits:
                caught[(T, tile)] = hits
    print(f"{mutation}: caught at {sorted(caught)}")
    at = lambda T, tile: caught.get((T, tile), [])
    if mutation == "drop_last_key":  # the last key takes all the weight under all_last, and is every mean's last term
        assert all("all_last" in at(T, tile) and "uniform" in at(T, tile) for T in ref.T_HOST for tile in TILES)
    elif mutation == "mask_off_by_one":  # a zero key has logit 0: only the uniform case weighs it, wherever the tail tile is not full
        assert all(("uniform" in at(T, tile)) == (T % tile != 0) for T in ref.T_HOST for tile in TILES)
    elif mutation == "no_rescale":  # the maximum arrives after the first tile: reversal and all_last, from two tiles on
        assert all(("reversal" in at(T, tile) and "all_last" in at(T, tile)) == (T > tile) for T in ref.T_HOST for tile in TILES)
    elif mutation == "store_tail_rows":
        assert all(bool(at(T, tile)) == (T % tile != 0) for T in ref.T_HOST for tile in TILES)
    else:
        assert all("identity" in at(T, tile) for T in ref.T_HOST for tile in TILES if T > 1)
    assert caught


def test_slice_errors_sees_what_the_whole_tensor_error_hides():
    heads, b, t = 2, 3, 8
    x = torch.randn((heads * 64, b, t), generator=torch.Generator().manual_seed(0)).double()
    x[64:, 1] *= 1e-3  # pair (b = 1, h = 1) is small
    y = x.clone()
    y[70, 1, 2] += 1e-6
    assert rel_err(y, x) < 1e-5
    err, pair = ref.slice_errors(y, x, heads)
    assert pair == 1 * heads + 1 and err > 1e-4
    lse = torch.zeros((b, heads, t)).double() + 1
    bad = lse.clone()
    bad[2, 0, 5] = float("nan")
    assert ref.slice_errors(bad, lse, heads) == (float("inf"), 2 * heads)
    nan_ref = lse.clone()
    nan_ref[2, 0] = float("nan")
    assert ref.slice_errors(lse, nan_ref, heads)[0] == 0.0


def _hand_masks(kind, heads, Bn, T, where, qkv):
    """The NaN masks IEEE arithmetic gives the attention formulas for each poison, derived by hand (see the GPU test's docstring)."""
    b, h = Bn - 1, heads - 1
    d, t = ref.POISON_CHANNEL, ref.poison_position(T, where)
    rows = slice(h * 64, (h + 1) * 64)
    m = {n: torch.zeros((heads * 64, Bn, T), dtype=torch.bool) for n in ("out", "dq", "dk", "dv")}
    m["lse"] = torch.zeros((Bn, heads, T), dtype=torch.bool)
    if kind == "q_nan":
        m["out"][rows, b, t] = m["dq"][rows, b, t] = True
        m["lse"][b, h, t] = True
        m["dk"][rows, b] = m["dv"][rows, b] = True
    elif kind == "k_nan":
        for n in ("out", "dq", "dk", "dv"):
            m[n][rows, b] = True
        m["lse"][b, h] = True
    elif kind == "v_nan":
        m["out"][h * 64 + d, b] = True
        m["dq"][rows, b] = m["dk"][rows, b] = True
    elif kind == "k_posinf":
        pos = qkv[h * 64 + d, b] > 0
        assert 0 < int(pos.sum()) < T
        m["out"][rows, b] = pos
        m["lse"][b, h] = pos
        m["dq"][rows, b] = pos
        m["dq"][h * 64 + d, b] = True  # 0 * Inf in the rows that stay finite
        m["dk"][rows, b] = m["dv"][rows, b] = True
    elif kind == "k_neginf_column":
        m["dq"][h * 64 + d, b] = True
    elif kind == "dout_nan":
        m["dq"][rows, b, t] = True
        m["dk"][rows, b] = True
        m["dv"][h * 64 + d, b] = True
    return m


@pytest.mark.parametrize("where", ["first", "tail"])
@pytest.mark.parametrize("kind", ref.POISONS)
def test_nonfinite_expectation_is_the_hand_derived_mask(kind, where):
    heads, Bn, T = 2, 2, 40
    qkv, dout, bad_qkv, bad_dout, (b, h) = ref.poison_case(kind, heads, Bn, T, where)
    assert (b, h) == (1, 1) and not torch.isnan(qkv).any() and torch.isfinite(dout).all()
    assert int((~torch.isfinite(bad_qkv)).sum()) + int((~torch.isfinite(bad_dout)).sum()) == 1
    exp = ref.nonfinite_expectation(bad_qkv, bad_dout, heads)
    want = _hand_masks(kind, heads, Bn, T, where, qkv)
    for name, mask in want.items():
        assert torch.equal(exp[name][1], mask), (kind, where, name, int(exp[name][1].sum()), int(mask.sum()))
        assert not torch.isinf(exp[name][0]).any(), name  # nothing is +-Inf: the masks say all
    clean = ref.attention_fp64(qkv, heads, ref.SCALE, dout)
    for name in want:  # the other pairs: the clean values
        keep = torch.arange(heads * Bn) != b * heads + h
        assert not ref.per_pair(want[name], heads)[keep].any()
        assert torch.equal(ref.per_pair(exp[name][0], heads)[keep], ref.per_pair(clean[name], heads)[keep])


def test_peaked_yardstick_e_cpu():
    """e_cpu of the GPU test's peaked inputs (scale 6.0): what fp32 torch autograd on the CPU loses against fp64.  Printed; the GPU
    test recomputes it and bounds the kernels by max(1e-5, 4 e_cpu)."""
    for heads, Bn, T in ref.PEAKED_SHAPES:
        qkv, dout = ref.peaked_inputs(heads, Bn, T)
        r = ref.attention_fp64(qkv, heads, ref.SCALE, dout)
        e = ref.cpu_fp32_yardstick(qkv, dout, heads, r)
        top = float(r["p"].max(dim=-1).values.mean())
        print(f"peaked heads={heads} B={Bn} T={T}: mean top weight {top:.2f}, e_cpu " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
        assert top > 0.5  # peaked indeed
        assert all(np.isfinite(v) and 1e-8 < v < 1e-4 for v in e.values())
