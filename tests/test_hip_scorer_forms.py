"""GPU tests of every dispatch form of the scorer's normalisation / depth-wise kernels (csrc/mgfn.hip: bn_rows, chan_layernorm,
chan_stats, head_ln_fc, dwconv_t, colsum) at the boundaries of each form, against the plain torch expression of the op in fp64.

Technique (the same for every op): the C entry points are called on test-owned buffers.  Every input is a view inside a larger
NaN-filled buffer (64 floats of NaN on either side: a read past an end poisons a sum), every output a view inside a sentinel-filled
one whose guard floats must keep their bits.  The same data one float further into its buffer is on a 4-byte boundary, which the
launchers answer with their generic / scalar form: every case runs aligned, with every operand misaligned, and with ONE operand
misaligned (taken in turn over the cases).  Each launch first asserts the library's form query for its own pointers
(tests/scorer_form_cases.py holds the expectations, tests/test_scorer_forms_host.py pins them without a GPU); all placements are
compared with fp64, and with each other within twice the bound (their sums associate differently: no equal bits asked).
Bounds: those of tests/test_hip_mgfn.py for the same ops.  Each case prints its forms and every measured rel_err."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import scorer_form_cases as cases
from conftest import rel_err
from anomaly_detection_on_video_amd.weights import synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
GUARD = 64          # floats of guard on either side of every operand (a multiple of 4: the aligned placement stays 16-byte aligned)
NAN = float("nan")
SENTINEL = -6.0e23  # what output buffers are filled with before a launch

SEEN = set()  # (query, the case's form when aligned, "aligned" / "misaligned"): what the launches asserted, counted by the last test
RAN = set()   # (query, case)


def _lib():
    from anomaly_detection_on_video_amd import _lib as m

    return m


def _bits(value):
    return int(torch.tensor([value], dtype=torch.float32).view(torch.int32))


class Buf:
    """A contiguous tensor inside a larger filled buffer.  data: an input (NaN around it); shape alone: an output (sentinel all
    over).  mis: one float further in, i.e. on a 4-byte boundary."""

    def __init__(self, data=None, mis=False, shape=None, guard=GUARD):
        fill = NAN if data is not None else SENTINEL
        shape = tuple(data.shape) if data is not None else tuple(shape)
        self.n = int(np.prod(shape))
        self.off = guard + (1 if mis else 0)
        self.raw = torch.full((self.n + 2 * guard + 4,), fill, device=DEV, dtype=torch.float32)
        assert guard % 4 == 0 and self.raw.data_ptr() % 16 == 0
        self.t = self.raw[self.off:self.off + self.n].view(shape)
        self.fill_bits = _bits(fill)
        if data is not None:
            self.t.copy_(data)
        assert self.t.is_contiguous() and (self.t.data_ptr() % 16 == 0) == (not mis) and self.t.data_ptr() % 4 == 0

    @property
    def p(self):
        return self.t.data_ptr()

    def guards_intact(self):
        g = torch.cat([self.raw[:self.off], self.raw[self.off + self.n:]]).view(torch.int32)
        return bool((g == self.fill_bits).all())

    def all_written(self):
        return not bool((self.t.reshape(-1).view(torch.int32) == self.fill_bits).any())


def Out(shape, mis=False, guard=GUARD):
    return Buf(shape=shape, mis=mis, guard=guard)


def _intact(**bufs):
    for name, b in bufs.items():
        assert b.guards_intact(), f"the guard floats around {name} changed"


def _written(**bufs):
    for name, b in bufs.items():
        assert b.all_written(), f"{name} still holds sentinel values"


def _placements(operands, index):
    """(name, the operands on a 4-byte boundary): none, all, and one of them alone -- another one for each case."""
    one = operands[index % len(operands)]
    return [("aligned", frozenset()), ("misaligned", frozenset(operands)), (f"only {one} misaligned", frozenset([one]))]


def _assert_form(what, shape, form, looked_at, names=None):
    """The form query's answer for THIS launch's pointers, asserted before the launch; returns it."""
    aligned16 = all(b.p % 16 == 0 for b in looked_at if b is not None)
    want = form if aligned16 else 0
    got = cases.query(_lib().load(), what, *shape, int(aligned16))
    assert got == want, f"{what}{shape} {'aligned' if aligned16 else 'misaligned'}: form {got}, the case is there for {want}"
    SEEN.add((what, form, "aligned" if aligned16 else "misaligned"))
    return (names or {}).get(got, str(got))


class Report:
    def __init__(self, head):
        self.head, self.items, self.forms = head, [], []

    def add(self, label, got, ref, bound):
        self.items.append((label, rel_err(got, ref), bound))

    def close(self):
        print(f"{self.head}: forms {'/'.join(self.forms)}; " + ", ".join(f"{l} {e:.2e}" for l, e, _ in self.items))
        bad = [(l, e, b) for l, e, b in self.items if not e < b]  # (a NaN fails)
        assert not bad, (self.head, bad)


def _agree(kept, bounds):
    """The placements of one case against each other: within twice the bound each holds against fp64."""
    base = kept["aligned"]
    for place, res in kept.items():
        for label, t in res.items():
            e = rel_err(t, base[label].double())
            assert e < 2 * bounds[label], (place, label, e)


def _stream(b):
    return _lib().stream(b.t)


def _dev64(t):
    return t.detach().double().to(DEV)


# ---- bn_rows ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _bn_ref(c, n):
    big = (c, n) == cases.BN_BIG_MEAN
    tag = f"{c}.{n}"
    inp = {
        "x": synth_tensor(f"sf.bn.x{tag}", (c, 1, n), scale=2.0, offset=80.0 if big else 0.3),
        "g": synth_tensor(f"sf.bn.g{tag}", (c,), scale=0.25, offset=1.0),
        "b": synth_tensor(f"sf.bn.b{tag}", (c,), scale=0.1),
        "dy": synth_tensor(f"sf.bn.dy{tag}", (c, 1, n), scale=1.0),
        "add": synth_tensor(f"sf.bn.add{tag}", (c, 1, n), scale=1.0),
        "rm0": synth_tensor(f"sf.bn.rm{tag}", (c,), scale=0.5, offset=0.2),
        "rv0": synth_tensor(f"sf.bn.rv{tag}", (c,), scale=0.5, offset=1.5),
    }
    xd, gd, bd = (inp[k].double().requires_grad_(True) for k in ("x", "g", "b"))
    ref = {}
    for m in (0.1, 1.0):
        rm, rv = inp["rm0"].double(), inp["rv0"].double()
        y = torch.nn.functional.batch_norm(xd.permute(1, 0, 2), rm, rv, gd, bd, training=True, momentum=m, eps=EPS).permute(1, 0, 2)
        ref[f"rm{m}"], ref[f"rv{m}"] = _dev64(rm), _dev64(rv)
    y.backward(inp["dy"].double())
    mean, var = xd.detach().mean(dim=(1, 2)), xd.detach().var(dim=(1, 2), unbiased=False)
    inp["mean"], inp["var"] = mean.float(), var.float()  # what the backward launches are given: the fp64 statistics, rounded
    ref.update(y=_dev64(y), mean=_dev64(mean), var=_dev64(var), dx=_dev64(xd.grad), dg=_dev64(gd.grad), db=_dev64(bd.grad),
               dx_add=_dev64(xd.grad + inp["add"].double()))
    return inp, ref


BN_BOUNDS = {"y": 1e-5, "mean": 1e-5, "var": 1e-5, "dx": 1e-4, "dgamma": 1e-4, "dbeta": 1e-5, "dx+add": 1e-4}


@pytest.mark.parametrize("c,n,form", cases.BN_CASES, ids=[f"{c}x{n}" for c, n, _ in cases.BN_CASES])
def test_bn_rows_forms_vs_fp64(c, n, form):
    """advhip_bn_rows_fwd_f32 / _fwd_running_f32 / _bwd_f32 / _bwd_add_f32 against torch.nn.functional.batch_norm(training=True) in
    fp64 autograd: y, batch mean, biased variance, the running statistics after one update at momentum 0.1 and 1.0 from non-trivial
    values, dx, dgamma, dbeta, and dx + add with `add` a buffer of its own (as _FocusAttnBlockCN.backward passes the incoming
    gradient; no caller passes dx itself as `add`)."""
    lib, f32 = _lib().load(), C.c_float
    inp, ref = _bn_ref(c, n)
    names = cases.BN_FORM_NAMES
    kept = {}
    for place, mis in _placements(("x", "y", "dy", "dx", "add"), cases.BN_CASES.index((c, n, form))):
        rep = Report(f"bn_rows C={c} N={n} {place}")
        x, g, b = Buf(inp["x"], "x" in mis), Buf(inp["g"]), Buf(inp["b"])
        y, mean, var = Out((c, 1, n), "y" in mis), Out((c,)), Out((c,))
        rep.forms.append("fwd " + _assert_form("bn_rows", (c, n), form, (x, y), names))
        _lib().check(lib.advhip_bn_rows_fwd_f32(x.p, g.p, b.p, y.p, mean.p, var.p, c, n, f32(EPS), _stream(x)), "bn_rows_fwd")
        rep.add("y", y.t, ref["y"], 1e-5)
        rep.add("mean", mean.t, ref["mean"], 1e-5)
        rep.add("var", var.t, ref["var"], 1e-5)
        _intact(x=x, g=g, b=b, y=y, mean=mean, var=var)
        _written(y=y, mean=mean, var=var)
        res = {"y": y.t, "mean": mean.t, "var": var.t}
        for m in (0.1, 1.0):
            y2, mean2, var2, rm, rv = Out((c, 1, n), "y" in mis), Out((c,)), Out((c,)), Buf(inp["rm0"]), Buf(inp["rv0"])
            _assert_form("bn_rows", (c, n), form, (x, y2), names)
            _lib().check(lib.advhip_bn_rows_fwd_running_f32(x.p, g.p, b.p, y2.p, mean2.p, var2.p, rm.p, rv.p, f32(m), c, n, f32(EPS), _stream(x)),
                         "bn_rows_fwd_running")
            assert torch.equal(y2.t, y.t) and torch.equal(mean2.t, mean.t) and torch.equal(var2.t, var.t)  # the same launch but for the update
            rep.add(f"running_mean(m={m})", rm.t, ref[f"rm{m}"], 1e-5)
            rep.add(f"running_var(m={m})", rv.t, ref[f"rv{m}"], 1e-5)
            _intact(x=x, y=y2, mean=mean2, var=var2, running_mean=rm, running_var=rv)
        dy, mean_in, var_in = Buf(inp["dy"], "dy" in mis), Buf(inp["mean"]), Buf(inp["var"])
        dx, dg, db = Out((c, 1, n), "dx" in mis), Out((c,)), Out((c,))
        rep.forms.append("bwd " + _assert_form("bn_rows", (c, n), form, (dy, x, dx), names))
        _lib().check(lib.advhip_bn_rows_bwd_f32(dy.p, x.p, g.p, mean_in.p, var_in.p, dx.p, dg.p, db.p, c, n, f32(EPS), _stream(x)), "bn_rows_bwd")
        rep.add("dx", dx.t, ref["dx"], 1e-4)
        rep.add("dgamma", dg.t, ref["dg"], 1e-4)
        rep.add("dbeta", db.t, ref["db"], 1e-5)
        _intact(dy=dy, x=x, g=g, mean=mean_in, var=var_in, dx=dx, dgamma=dg, dbeta=db)
        _written(dx=dx, dgamma=dg, dbeta=db)
        add, dx2, dg2, db2 = Buf(inp["add"], "add" in mis), Out((c, 1, n), "dx" in mis), Out((c,)), Out((c,))
        rep.forms.append("bwd_add " + _assert_form("bn_rows", (c, n), form, (dy, x, dx2, add), names))
        _lib().check(lib.advhip_bn_rows_bwd_add_f32(dy.p, x.p, g.p, mean_in.p, var_in.p, add.p, dx2.p, dg2.p, db2.p, c, n, f32(EPS), _stream(x)),
                     "bn_rows_bwd_add")
        rep.add("dx+add", dx2.t, ref["dx_add"], 1e-4)
        rep.add("dgamma(add)", dg2.t, ref["dg"], 1e-4)
        rep.add("dbeta(add)", db2.t, ref["db"], 1e-5)
        _intact(dy=dy, x=x, add=add, dx=dx2, dgamma=dg2, dbeta=db2)
        _written(dx=dx2, dgamma=dg2, dbeta=db2)
        res.update({"dx": dx.t, "dgamma": dg.t, "dbeta": db.t, "dx+add": dx2.t})
        kept[place] = res
        rep.close()
    _agree(kept, BN_BOUNDS)
    RAN.add(("bn_rows", (c, n)))


@pytest.mark.parametrize("momentum", [0.1, 1.0])
def test_bn_rows_running_statistics_of_a_single_position(momentum):
    """N = 1, where torch refuses to train: what the kernel documents -- the batch variance is 0 and its N / (N - 1) factor is
    guarded, so y = beta, running_var takes momentum * 0, running_mean momentum * x, and everything stays finite."""
    lib, f32, c = _lib().load(), C.c_float, 5
    xs, gs, bs = synth_tensor("sf.bn1.x", (c, 1, 1), scale=2.0, offset=0.3), synth_tensor("sf.bn1.g", (c,), scale=0.25, offset=1.0), synth_tensor("sf.bn1.b", (c,), scale=0.1)
    rm0, rv0 = synth_tensor("sf.bn1.rm", (c,), scale=0.5, offset=0.2), synth_tensor("sf.bn1.rv", (c,), scale=0.5, offset=1.5)
    x, g, b, rm, rv = Buf(xs), Buf(gs), Buf(bs), Buf(rm0), Buf(rv0)
    y, mean, var = Out((c, 1, 1)), Out((c,)), Out((c,))
    assert _assert_form("bn_rows", (c, 1), cases.BN_GENERIC, (x, y)) == "0"
    _lib().check(lib.advhip_bn_rows_fwd_running_f32(x.p, g.p, b.p, y.p, mean.p, var.p, rm.p, rv.p, f32(momentum), c, 1, f32(EPS), _stream(x)), "bn_rows_fwd_running")
    _intact(x=x, g=g, b=b, y=y, mean=mean, var=var, running_mean=rm, running_var=rv)
    got = [t.t.cpu() for t in (y, mean, var, rm, rv)]
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert torch.equal(got[1], xs.view(-1)) and not got[2].any()
    assert torch.equal(got[0].view(-1), bs)  # (x - mean) * sc + beta with x - mean = 0: beta itself, not beta within the rounding of x * sc
    m = float(np.float32(momentum))
    assert rel_err(got[3], (1 - m) * rm0.double() + m * xs.view(-1).double()) < 1e-5
    assert rel_err(got[4], (1 - m) * rv0.double()) < 1e-5
    print(f"bn_rows N=1 momentum {momentum}: y - beta {rel_err(got[0].view(-1), bs.double()):.2e}")


# ---- chan_layernorm / chan_stats -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _ln_ref(c, n):
    big = (c, n) == cases.LN_BIG_MEAN
    tag = f"{c}.{n}"
    inp = {
        "x": synth_tensor(f"sf.ln.x{tag}", (c, 1, n), scale=2.0, offset=80.0 if big else 0.7),
        "g": synth_tensor(f"sf.ln.g{tag}", (c,), scale=0.25, offset=1.0),
        "b": synth_tensor(f"sf.ln.b{tag}", (c,), scale=0.1),
        "dy": synth_tensor(f"sf.ln.dy{tag}", (c, 1, n), scale=1.0),
        "add": synth_tensor(f"sf.ln.add{tag}", (c, 1, n), scale=1.0),
    }
    xd, gd, bd = (inp[k].double().requires_grad_(True) for k in ("x", "g", "b"))
    var, mean = torch.var_mean(xd, dim=0, unbiased=False, keepdim=True)
    y = (xd - mean) / (var.sqrt() + EPS) * gd.view(-1, 1, 1) + bd.view(-1, 1, 1)
    y.backward(inp["dy"].double())
    mu, rs = mean.detach().reshape(n), (1.0 / (var.detach().sqrt() + EPS)).reshape(n)
    inp["mu"], inp["rs"] = mu.float(), rs.float()  # what the backward launches are given
    ref = dict(y=_dev64(y), mu=_dev64(mu), rs=_dev64(rs), dx=_dev64(xd.grad), dg=_dev64(gd.grad), db=_dev64(bd.grad),
               dx_add=_dev64(xd.grad + inp["add"].double()))
    return inp, ref


LN_BOUNDS = {"y": 1e-5, "mu": 1e-5, "rs": 1e-5, "dx": 1e-4, "dg": 1e-4, "db": 1e-5, "dx+add": 1e-4}


@pytest.mark.parametrize("c,n,form", cases.LN_CASES, ids=[f"{c}x{n}" for c, n, _ in cases.LN_CASES])
def test_chan_layernorm_forms_vs_fp64(c, n, form):
    """advhip_chan_layernorm_fwd_f32 / _bwd_f32 / _bwd_add_f32 and advhip_chan_stats_f32 against MGFNLayerNorm's formula
    ((x - mean) / (sqrt(var_biased) + eps) * g + b over the channels) in fp64 autograd.  dg / db are the per-block partial-sum rows
    reduced by advhip_colsum_f32: [rows][C] twice for _bwd, one [rows][2C] matrix with dg | db for _bwd_add; nothing behind
    partial_rows(N) rows is written.  N % 32 != 0 leaves the last block partly (N = 4: mostly) empty."""
    from anomaly_detection_on_video_amd import mgfn_ops

    lib, f32 = _lib().load(), C.c_float
    inp, ref = _ln_ref(c, n)
    rows = int(lib.advhip_chan_layernorm_bwd_partial_rows(n))
    assert rows == -(-n // 32)
    pguard = -(-2 * 2 * c // 4) * 4  # two whole rows of the widest partial matrix on either side
    kept = {}
    for place, mis in _placements(("x", "y", "mu", "rs", "dy", "dx", "add"), cases.LN_CASES.index((c, n, form))):
        rep = Report(f"chan_layernorm C={c} N={n} {place}")
        x, g, b = Buf(inp["x"], "x" in mis), Buf(inp["g"]), Buf(inp["b"])
        y, mu, rs = Out((c, 1, n), "y" in mis), Out((n,), "mu" in mis), Out((n,), "rs" in mis)
        rep.forms.append("fwd " + _assert_form("chan_layernorm", (c, n), form, (x, y, mu, rs)))
        _lib().check(lib.advhip_chan_layernorm_fwd_f32(x.p, g.p, b.p, y.p, mu.p, rs.p, c, n, f32(EPS), _stream(x)), "chan_layernorm_fwd")
        rep.add("y", y.t, ref["y"], 1e-5)
        rep.add("mu", mu.t, ref["mu"], 1e-5)
        rep.add("rs", rs.t, ref["rs"], 1e-5)
        _intact(x=x, g=g, b=b, y=y, mu=mu, rs=rs)
        _written(y=y, mu=mu, rs=rs)
        smu, srs = Out((n,), "mu" in mis), Out((n,), "rs" in mis)
        _lib().check(lib.advhip_chan_stats_f32(x.p, smu.p, srs.p, c, n, f32(EPS), _stream(x)), "chan_stats")
        rep.add("stats mu", smu.t, ref["mu"], 1e-5)
        rep.add("stats rs", srs.t, ref["rs"], 1e-5)
        _intact(x=x, mu=smu, rs=srs)
        _written(mu=smu, rs=srs)
        dy, mu_in, rs_in = Buf(inp["dy"], "dy" in mis), Buf(inp["mu"], "mu" in mis), Buf(inp["rs"], "rs" in mis)
        dx, pg, pb = Out((c, 1, n), "dx" in mis), Out((rows, c), guard=pguard), Out((rows, c), guard=pguard)
        rep.forms.append("bwd " + _assert_form("chan_layernorm", (c, n), form, (dy, x, dx, mu_in, rs_in)))
        _lib().check(lib.advhip_chan_layernorm_bwd_f32(dy.p, x.p, g.p, mu_in.p, rs_in.p, dx.p, pg.p, pb.p, c, n, f32(EPS), _stream(x)), "chan_layernorm_bwd")
        _intact(dy=dy, x=x, g=g, mu=mu_in, rs=rs_in, dx=dx, dg_partial=pg, db_partial=pb)
        _written(dx=dx, dg_partial=pg, db_partial=pb)
        dg, db = mgfn_ops.colsum(pg.t), mgfn_ops.colsum(pb.t)
        rep.add("dx", dx.t, ref["dx"], 1e-4)
        rep.add("dg", dg, ref["dg"], 1e-4)
        rep.add("db", db, ref["db"], 1e-5)
        add, dx2, pgb = Buf(inp["add"], "add" in mis), Out((c, 1, n), "dx" in mis), Out((rows, 2 * c), guard=pguard)
        rep.forms.append("bwd_add " + _assert_form("chan_layernorm", (c, n), form, (dy, x, dx2, mu_in, rs_in, add)))
        _lib().check(lib.advhip_chan_layernorm_bwd_add_f32(dy.p, x.p, g.p, mu_in.p, rs_in.p, add.p, dx2.p, pgb.p, c, n, f32(EPS), _stream(x)),
                     "chan_layernorm_bwd_add")
        _intact(dy=dy, x=x, add=add, mu=mu_in, rs=rs_in, dx=dx2, dgb_partial=pgb)
        _written(dx=dx2, dgb_partial=pgb)
        dgb = mgfn_ops.colsum(pgb.t)
        rep.add("dx+add", dx2.t, ref["dx_add"], 1e-4)
        rep.add("[dg|", dgb[:c], ref["dg"], 1e-4)
        rep.add("|db]", dgb[c:], ref["db"], 1e-5)
        kept[place] = {"y": y.t, "mu": mu.t, "rs": rs.t, "dx": dx.t, "dg": dg, "db": db, "dx+add": dx2.t}
        rep.close()
    _agree(kept, LN_BOUNDS)
    RAN.add(("chan_layernorm", (c, n)))


# ---- head_ln_fc ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _head_ref(c, n, saturated):
    big = (c, n) == cases.HEAD_BIG_MEAN and not saturated
    tag = f"{c}.{n}"
    inp = {
        "y": synth_tensor(f"sf.hd.y{tag}", (c, 1, n), scale=2.0, offset=80.0 if big else 0.3),
        "g": synth_tensor(f"sf.hd.g{tag}", (c,), scale=0.25, offset=1.0),
        "b": synth_tensor(f"sf.hd.b{tag}", (c,), scale=0.1),
        "w": synth_tensor(f"sf.hd.w{tag}", (1, c), scale=float(c) ** -0.5),
        "b0": synth_tensor(f"sf.hd.b0{tag}", (1,), scale=0.1),
        "gx": synth_tensor(f"sf.hd.gx{tag}", (1, n, c), scale=1.0),
        "gs": synth_tensor(f"sf.hd.gs{tag}", (1, n, 1), scale=1.0),
    }
    ln64, fc64 = torch.nn.LayerNorm(c, eps=EPS).double(), torch.nn.Linear(c, 1).double()
    if saturated:  # fc_w scaled so that the largest |logit - fc_b| is 30
        with torch.no_grad():
            xn = torch.nn.functional.layer_norm(inp["y"].double().permute(1, 2, 0), (c,), inp["g"].double(), inp["b"].double(), EPS)
            inp["w"] = (inp["w"].double() * (30.0 / float((xn @ inp["w"].double().t()).abs().max()))).float()
    ln64.load_state_dict({"weight": inp["g"].double(), "bias": inp["b"].double()})
    fc64.load_state_dict({"weight": inp["w"].double(), "bias": inp["b0"].double()})
    y64 = inp["y"].double().requires_grad_(True)
    x_ref = ln64(y64.permute(1, 2, 0))
    logit = fc64(x_ref)
    s_ref = torch.sigmoid(logit)
    (x_ref * inp["gx"].double()).sum().add((s_ref * inp["gs"].double()).sum()).backward()
    mean = y64.detach().mean(dim=0).reshape(n)
    rstd = (y64.detach().var(dim=0, unbiased=False) + EPS).rsqrt().reshape(n)
    inp["mean"], inp["rstd"], inp["score"] = mean.float(), rstd.float(), s_ref.detach().reshape(n).float()
    ref = dict(xn=_dev64(x_ref), score=_dev64(s_ref.reshape(n)), mean=_dev64(mean), rstd=_dev64(rstd), dy=_dev64(y64.grad), dg=_dev64(ln64.weight.grad),
               db=_dev64(ln64.bias.grad), dw=_dev64(fc64.weight.grad.reshape(c)), db0=_dev64(fc64.bias.grad), max_logit=float(logit.detach().abs().max()))
    return inp, ref


HEAD_BOUNDS = {"xn": 1e-5, "score": 1e-5, "dy": 2e-5, "dg": 2e-5, "db": 2e-5, "dw": 2e-5, "db0": 2e-5}


def _head_case(c, n, form, saturated):
    from anomaly_detection_on_video_amd import mgfn_ops

    lib, f32 = _lib().load(), C.c_float
    inp, ref = _head_ref(c, n, saturated)
    if saturated:
        assert 29.9 < ref["max_logit"] < 30.2
    rows = int(lib.advhip_head_ln_fc_partial_rows(n))
    assert rows == -(-n // 32)
    width = 3 * c + 1
    pguard = -(-2 * width // 4) * 4
    kept = {}
    index = [row[:2] for row in cases.HEAD_CASES].index((c, n)) + (3 if saturated else 0)
    for place, mis in _placements(("y", "xn", "mean", "rstd", "score", "d_xn", "d_score", "dy"), index):
        rep = Report(f"head_ln_fc C={c} N={n}{' saturated' if saturated else ''} {place}")
        y, g, b, w, b0 = Buf(inp["y"], "y" in mis), Buf(inp["g"]), Buf(inp["b"]), Buf(inp["w"]), Buf(inp["b0"])
        xn, mean, rstd, score = Out((1, n, c), "xn" in mis), Out((n,), "mean" in mis), Out((n,), "rstd" in mis), Out((n,), "score" in mis)
        rep.forms.append("fwd " + _assert_form("head_ln_fc", (c, n), form, (y, xn, mean, rstd, score)))
        _lib().check(lib.advhip_head_ln_fc_fwd_f32(y.p, g.p, b.p, w.p, b0.p, xn.p, mean.p, rstd.p, score.p, c, n, f32(EPS), _stream(y)), "head_ln_fc_fwd")
        rep.add("xn", xn.t, ref["xn"], 1e-5)
        rep.add("score", score.t, ref["score"], 1e-5)
        rep.add("mean", mean.t, ref["mean"], 1e-5)
        rep.add("rstd", rstd.t, ref["rstd"], 1e-5)
        _intact(y=y, g=g, b=b, w=w, b0=b0, xn=xn, mean=mean, rstd=rstd, score=score)
        _written(xn=xn, mean=mean, rstd=rstd, score=score)
        gx, gs = Buf(inp["gx"], "d_xn" in mis), Buf(inp["gs"].reshape(n), "d_score" in mis)
        mean_in, rstd_in, score_in = Buf(inp["mean"], "mean" in mis), Buf(inp["rstd"], "rstd" in mis), Buf(inp["score"], "score" in mis)
        dy, partial = Out((c, 1, n), "dy" in mis), Out((rows, width), guard=pguard)
        rep.forms.append("bwd " + _assert_form("head_ln_fc", (c, n), form, (y, gx, gs, mean_in, rstd_in, score_in, dy)))
        _lib().check(lib.advhip_head_ln_fc_bwd_f32(gx.p, gs.p, y.p, g.p, b.p, w.p, mean_in.p, rstd_in.p, score_in.p, dy.p, partial.p, c, n, _stream(y)),
                     "head_ln_fc_bwd")
        _intact(d_xn=gx, d_score=gs, y=y, mean=mean_in, rstd=rstd_in, score=score_in, dy=dy, partial=partial)
        _written(dy=dy, partial=partial)
        sums = mgfn_ops.colsum(partial.t)
        assert bool(torch.isfinite(dy.t).all()) and bool(torch.isfinite(sums).all())
        res = {"xn": xn.t, "score": score.t, "dy": dy.t, "dg": sums[:c], "db": sums[c:2 * c], "dw": sums[2 * c:3 * c], "db0": sums[3 * c:]}
        for label in ("dy", "dg", "db", "dw", "db0"):
            rep.add(label, res[label], ref[label], 2e-5)
        kept[place] = res
        rep.close()
    _agree(kept, HEAD_BOUNDS)


@pytest.mark.parametrize("c,n,form", cases.HEAD_CASES, ids=[f"{c}x{n}" for c, n, _ in cases.HEAD_CASES])
def test_head_ln_fc_forms_vs_fp64(c, n, form):
    """advhip_head_ln_fc_fwd_f32 / _bwd_f32 against nn.LayerNorm(C) + nn.Linear(C, 1) + sigmoid in fp64 autograd, gradients flowing
    in through xn AND through the scores: xn, score, the saved statistics, the input gradient and the four parameter gradients
    (the [rows][3C + 1] partial sums reduced by advhip_colsum_f32)."""
    _head_case(c, n, form, False)
    RAN.add(("head_ln_fc", (c, n)))


def test_head_ln_fc_saturated_logits_vs_fp64():
    """Logits up to +-30 (fc_w scaled): the score gradient s (1 - s) underflows towards 0 on both sides, must match fp64 and
    stay finite -- in the 16-byte form and in the generic one."""
    c, n = cases.HEAD_SATURATED
    _head_case(c, n, 1, True)


# ---- dwconv_t ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _dw_ref(k, t, c, heads, rows):
    big = (k, t) == cases.DW_BIG_MEAN
    tag = f"{k}.{t}.{rows}"
    inp = {
        "v": synth_tensor(f"sf.dw.v{tag}", (c, rows, t), scale=2.0 if big else 1.5, offset=80.0 if big else 0.0),
        "w": synth_tensor(f"sf.dw.w{tag}", (heads, 1, k), scale=0.5),
        "bias": synth_tensor(f"sf.dw.b{tag}", (heads,), scale=0.2),
        "dout": synth_tensor(f"sf.dw.d{tag}", (c, rows, t), scale=1.0),
    }
    vd, wd, bd = (inp[n].double().requires_grad_(True) for n in ("v", "w", "bias"))
    xr = vd.permute(1, 0, 2).reshape(rows, c // heads, heads, t).reshape(rows * (c // heads), heads, t)
    yr = torch.nn.functional.conv1d(xr, wd, bd, padding=k // 2, groups=heads)
    out = yr.reshape(rows, c // heads, heads, t).reshape(rows, c, t).permute(1, 0, 2)
    out.backward(inp["dout"].double())
    return inp, dict(out=_dev64(out), dv=_dev64(vd.grad), dw=_dev64(wd.grad.reshape(heads, k)), db=_dev64(bd.grad))


DW_BOUNDS = {"out": 1e-5, "dv": 1e-5, "dw": 1e-4, "db": 1e-4}


@pytest.mark.parametrize("k,t,form", cases.DW_CASES, ids=[f"K{k}-T{t}" for k, t, _ in cases.DW_CASES])
def test_dwconv_t_forms_vs_fp64(k, t, form):
    """advhip_dwconv_t_fwd_f32 / _bwd_f32 against the reference formulation ('b (c h) n -> (b c) h n', Conv1d(heads, heads, K,
    padding=K//2, groups=heads)) in fp64 autograd, on geometries whose backward runs 1, 2, 4 and 32 chunks per channel; the filter
    and bias gradients from the partial sums through advhip_colsum_f32, as _DWConvT.backward takes them.  T = 4: the one quad
    of a row has no neighbour on either side; T = 8: each quad has one."""
    from anomaly_detection_on_video_amd import mgfn_ops

    lib = _lib().load()
    case = cases.DW_CASES.index((k, t, form))
    for gi, (c, heads, rows, chunks) in enumerate(cases.DW_GEOMETRIES):
        assert lib.advhip_dwconv_t_bwd_chunks(c, rows) == chunks
        inp, ref = _dw_ref(k, t, c, heads, rows)
        kept = {}
        for place, mis in _placements(("v", "out", "dout", "dv"), case + gi):
            rep = Report(f"dwconv_t K={k} T={t} (C, H, rows)=({c}, {heads}, {rows}) chunks={chunks} {place}")
            v, w, bias = Buf(inp["v"], "v" in mis), Buf(inp["w"].reshape(heads, k)), Buf(inp["bias"])
            out = Out((c, rows, t), "out" in mis)
            rep.forms.append("fwd " + _assert_form("dwconv_t", (t,), form, (v, out)))
            _lib().check(lib.advhip_dwconv_t_fwd_f32(v.p, w.p, bias.p, out.p, c, heads, rows, t, k, _stream(v)), "dwconv_t_fwd")
            rep.add("out", out.t, ref["out"], 1e-5)
            _intact(v=v, w=w, bias=bias, out=out)
            _written(out=out)
            dout, dv, partial = Buf(inp["dout"], "dout" in mis), Out((c, rows, t), "dv" in mis), Out((c * chunks, k + 1))
            rep.forms.append("bwd " + _assert_form("dwconv_t", (t,), form, (dout, v, dv)))
            _lib().check(lib.advhip_dwconv_t_bwd_f32(dout.p, v.p, w.p, dv.p, partial.p, c, heads, rows, t, k, _stream(v)), "dwconv_t_bwd")
            _intact(dout=dout, v=v, w=w, dv=dv, partial=partial)
            _written(dv=dv, partial=partial)
            per_head = mgfn_ops.colsum(partial.t.view(c // heads * chunks, heads * (k + 1))).view(heads, k + 1)
            res = {"out": out.t, "dv": dv.t, "dw": per_head[:, :k], "db": per_head[:, k]}
            rep.add("dv", res["dv"], ref["dv"], 1e-5)
            rep.add("dw", res["dw"], ref["dw"], 1e-4)
            rep.add("db", res["db"], ref["db"], 1e-4)
            kept[place] = res
            rep.close()
        _agree(kept, DW_BOUNDS)
    RAN.add(("dwconv_t", (k, t)))


# ---- colsum / colsum_group -------------------------------------------------------------------------------------------------------

def _colsum_check(got, src64, rows, what):
    """|got - ref| <= 2^-23 (rows / 8 + 8) sum_r |src[r][c]| per column: the kernel's longest chain of fp32 additions is a thread's
    ceil(rows / 8) rows, then the 8 row groups."""
    ref = src64.sum(0)
    bound = 2.0 ** -23 * (rows / 8 + 8) * src64.abs().sum(0)
    err = (got.double().cpu() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), (what, worst)
    return worst


@pytest.mark.parametrize("rows", cases.COLSUM_ROWS)
def test_colsum_and_colsum_group_vs_fp64(rows):
    """advhip_colsum_f32 and advhip_colsum_group_f32 against fp64 column sums with a derived bound (not a measured one): row counts
    around the 8-at-a-time body (it needs r + 56 < rows) and the 8 row groups, column counts around the 32-column block, and
    `period`: the de-interleaved destination order against the plain permutation."""
    lib, m = _lib().load(), _lib()
    worst = 0.0
    singles = []
    for cols in cases.COLSUM_COLS:
        data = synth_tensor(f"sf.cs.{rows}.{cols}", (rows, cols), scale=1.0, offset=0.25)
        src, dst = Buf(data), Out((cols,))
        m.check(lib.advhip_colsum_f32(src.p, dst.p, rows, cols, _stream(src)), "colsum")
        _intact(src=src, dst=dst)
        _written(dst=dst)
        worst = max(worst, _colsum_check(dst.t, data.double(), rows, ("colsum", rows, cols)))
        singles.append((data, src, 0, dst.t.clone()))
    group = [(d, s, 0, got) for d, s, _p, got in singles]
    for cols in cases.COLSUM_PERIOD_COLS:
        for period in cases.COLSUM_PERIODS:
            data = synth_tensor(f"sf.cs.{rows}.{cols}.{period}", (rows, cols), scale=1.0, offset=0.25)
            group.append((data, Buf(data), period, None))
    arr = (m.ColsumItem * len(group))()
    dsts = [Out((d.shape[1],)) for d, _s, _p, _g in group]
    for it, (data, src, period, _g), dst in zip(arr, group, dsts):
        it.src, it.dst, it.rows, it.cols, it.period = src.p, dst.p, rows, data.shape[1], period
    m.check(lib.advhip_colsum_group_f32(arr, len(group), _stream(dsts[0])), "colsum_group")
    for (data, src, period, single), dst in zip(group, dsts):
        cols = data.shape[1]
        _intact(src=src, dst=dst)
        _written(dst=dst)
        if period == 0:
            assert torch.equal(dst.t, single)  # the same body as the single launch
            continue
        heads = cols // period
        # where the plain permutation puts column h * period + j: the first period - 1 of every group, group after group, then the last ones
        order = np.concatenate([np.arange(cols).reshape(heads, period)[:, :period - 1].reshape(-1), np.arange(cols).reshape(heads, period)[:, period - 1]])
        worst = max(worst, _colsum_check(dst.t, data.double()[:, torch.from_numpy(order)], rows, ("colsum_group", rows, cols, period)))
    print(f"colsum rows={rows}: worst |err| / bound {worst:.3f}")


# ---- the count -------------------------------------------------------------------------------------------------------------------

def test_every_form_of_every_query_was_asserted_in_both_placements():
    """Counts what the launches above asserted against the full list of forms: every form's cases ran aligned (the query answered
    that form) and with operands on a 4-byte boundary (the query answered the generic form).  Runs last; with a part of the file
    deselected it counts the forms of the cases that did run."""
    all_cases = ({("bn_rows", (c, n)) for c, n, _ in cases.BN_CASES} | {("chan_layernorm", (c, n)) for c, n, _ in cases.LN_CASES}
                 | {("head_ln_fc", (c, n)) for c, n, _ in cases.HEAD_CASES} | {("dwconv_t", (k, t)) for k, t, _ in cases.DW_CASES})
    forms = {"bn_rows": {(c, n): f for c, n, f in cases.BN_CASES}, "chan_layernorm": {(c, n): f for c, n, f in cases.LN_CASES},
             "head_ln_fc": {(c, n): f for c, n, f in cases.HEAD_CASES}, "dwconv_t": {(k, t): f for k, t, f in cases.DW_CASES}}
    assert RAN <= all_cases
    expected = {(what, forms[what][shape], place) for what, shape in RAN for place in ("aligned", "misaligned")}
    print(f"{len(RAN)} of {len(all_cases)} cases ran; forms asserted: {sorted(SEEN)}")
    assert expected <= SEEN, sorted(expected - SEEN)
    if RAN == all_cases:
        full = {(what, f, place) for what, f in cases.ALL_FORMS for place in ("aligned", "misaligned")}
        assert SEEN == full, sorted(SEEN ^ full)
        assert len(full) == 2 * len(cases.ALL_FORMS) == 24
