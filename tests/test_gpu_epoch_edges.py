"""The dealt-epoch kernels (glove_masters_build, glove_epoch_deal, glove_plan_build_sorted) at every tile, digit and pass
edge of tests/epoch_cases.py, bit for bit against oracle/glove_ref.py (build_masters / deal_epoch / build_plan): integer work,
no tolerances.  tests/test_epoch_cases.py proves on the CPU that every case reaches the branch its label names and pins the
oracle functions used here."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import epoch_cases as ec
import glove_ref as ref
from epoch_cases import KEY, T
from helpers import PLAN_ARRAYS, _assert_plan_equals_oracle, _poison

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BADARG, WORKSPACE = -1, -2          # GLOVE_E_BADARG, GLOVE_E_WORKSPACE (include/glove_hip.h)
GUARD = 64                          # elements behind n of every output array of a deal
WS_GUARD = 256                      # bytes behind the queried workspace size
PAIR_FIELDS = ("id", "partner", "w", "y")
label = lambda c: c.label           # noqa: E731


def _dev(*arrays):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in arrays]


def _pairs(n, extra=0):
    """A Pairs of n pairs whose arrays hold `extra` more elements behind them."""
    from trainer.hip_api import Pairs
    p = Pairs(n + extra, DEV)
    p.n = n
    return p


def _pairs_from(arrays):
    p = _pairs(len(arrays[0]))
    for f, a in zip(PAIR_FIELDS, arrays):
        getattr(p, f).copy_(torch.from_numpy(np.array(a)))
    return p


def _fill(pairs, byte):
    for f in PAIR_FIELDS:
        getattr(pairs, f).view(torch.uint8).fill_(byte)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _snapshot(*pairs, more=()):
    return [_bits(getattr(p, f)).clone() for p in pairs for f in PAIR_FIELDS] + [_bits(t).clone() for t in more]


def _same(snap, *pairs, more=()):
    now = [_bits(getattr(p, f)) for p in pairs for f in PAIR_FIELDS] + [_bits(t) for t in more]
    return all(torch.equal(a, b) for a, b in zip(snap, now))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _assert_masters(m, want, w, y, n):
    """What test_masters_are_the_two_sorted_orders asserts: id, partner, w, y of both orders and the link."""
    for pairs, perm, own, other in ((m.row_major, want["perm_r"], want["row"], want["col"]),
                                    (m.col_major, want["perm_c"], want["col"], want["row"])):
        np.testing.assert_array_equal(pairs.id.cpu().numpy()[:n], own[perm])
        np.testing.assert_array_equal(pairs.partner.cpu().numpy()[:n], other[perm])
        np.testing.assert_array_equal(pairs.w.cpu().numpy()[:n], w[perm])
        np.testing.assert_array_equal(pairs.y.cpu().numpy()[:n], y[perm])
    np.testing.assert_array_equal(m.link.cpu().numpy()[:n], want["link"])


def _assert_epoch(rs, cs, want_m, w, y, ir, ic, n):
    for side, idx, own, other in ((rs, ir, "row", "col"), (cs, ic, "col", "row")):
        np.testing.assert_array_equal(side.id.cpu().numpy()[:n], want_m[own][idx])
        np.testing.assert_array_equal(side.partner.cpu().numpy()[:n], want_m[other][idx])
        np.testing.assert_array_equal(side.w.cpu().numpy()[:n], w[idx])
        np.testing.assert_array_equal(side.y.cpu().numpy()[:n], y[idx])


def _guards_intact(*pairs):
    return all(bool((getattr(p, f).view(torch.uint8)[4 * p.n:] == 0xFF).all()) for p in pairs for f in PAIR_FIELDS)


# ---- glove_masters_build -----------------------------------------------------------------------------------------------
def test_masters_of_an_empty_stream(hip):
    """n = 0 returns at once: nothing is read or written but the count of mapped ids, which is 0."""
    from trainer.hip_api import Pairs
    rm, cm = Pairs(0, DEV), Pairs(0, DEV)
    _fill(rm, 0xFF); _fill(cm, 0xFF)
    mapped = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    rc = hip.lib.glove_masters_build(None, None, None, None, 0, 5, 0, C.byref(rm.struct()), C.byref(cm.struct()), None,
                                     mapped.data_ptr(), None, 0, _stream())
    assert rc == 0 and mapped.item() == 0
    assert _guards_intact(rm, cm)
    empty_i, empty_f = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, dtype=torch.float32, device=DEV)
    m = hip.build_masters(empty_i, empty_i, empty_f, empty_f, 5)
    assert m.mapped == 0 and m.n == 0


@pytest.mark.parametrize("case", ec.MASTERS_CASES, ids=label)
def test_masters_at_the_edges(hip, case):
    """Both master orders and their link at one position, one tile +- 1, a partial last wave, one / two / three passes per
    field, a pass that covers no bits of one order, one digit that takes every tile, all keys equal (stream order, link the
    identity), three distinct pairs (stable in w) and ids at the ends of int32, at V and at V_row (they count as id 0)."""
    row, col, w, y = ec.masters_stream(case.n, case.V, case.V_row, case.ids)
    m = hip.build_masters(*_dev(row, col, w, y), case.V, case.V_row)
    want = ref.build_masters(row, col, case.V, case.V_row or None)
    assert m.mapped == ec.mapped_count(row, col, case.V, case.V_row)
    _assert_masters(m, want, w, y, case.n)


# ---- glove_epoch_deal ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.DEAL_CASES, ids=label)
def test_deal_at_the_edges(hip, case):
    """One epoch per key: pair for pair oracle.deal_epoch; nothing written behind n or behind the workspace; the same bits
    whatever the workspace held before; the masters untouched; the deal repeatable into the same buffers."""
    n, B, V = case.n, case.B, case.V
    row, col, w, y = ec.masters_stream(n, V)
    m = hip.build_masters(*_dev(row, col, w, y), V)
    want_m = ref.build_masters(row, col, V)
    _assert_masters(m, want_m, w, y, n)
    before = _snapshot(m.row_major, m.col_major, more=(m.link,))
    rs, cs = _pairs(n, GUARD), _pairs(n, GUARD)
    size = hip.lib.glove_epoch_deal_workspace_bytes(n, B)
    assert size > 0
    ws_full = torch.empty(size + WS_GUARD, dtype=torch.uint8, device=DEV)
    ws = ws_full[:size]
    for key in case.keys:
        ir, ic = ref.deal_epoch(want_m, B, key)
        first = None
        for fill in (0xFF, 0x00):
            ws.fill_(fill)
            ws_full[size:].fill_(0xA5)
            _fill(rs, 0xFF); _fill(cs, 0xFF)
            hip.deal_epoch(m, B, key, rs, cs, ws)
            assert _guards_intact(rs, cs), "written behind n"
            assert bool((ws_full[size:] == 0xA5).all()), "written behind the workspace"
            if first is None:
                _assert_epoch(rs, cs, want_m, w, y, ir, ic, n)
                first = _snapshot(rs, cs)
            else:
                assert _same(first, rs, cs), "the deal depends on what its workspace held"
        hip.deal_epoch(m, B, key, rs, cs, ws)               # again, into the buffers as they are
        assert _same(first, rs, cs) and _guards_intact(rs, cs)
    assert _same(before, m.row_major, m.col_major, more=(m.link,)), "the deal wrote into the masters"


# ---- glove_plan_build_sorted ---------------------------------------------------------------------------------------------
def _sorted_ws(hip, B, nb):
    return torch.empty(max(hip.lib.glove_plan_sorted_workspace_bytes(B, nb), 256), dtype=torch.uint8, device=DEV)


def _block(hip, B, V, cap, kind, nb, V_row=0):
    from trainer.hip_api import PlanBlock
    block = PlanBlock([hip.staging_plan(B, V, cap, DEV, V_row=V_row, **ec.plan_kind_args(kind)) for _ in range(nb)])
    p = block.plans[0]
    assert (p.r_crec is not None) == (kind == "records") and (p.r_chunk_hw is not None) == (kind != "records")
    assert (p.r_partner is not None) == (kind == "words") and p.c_perm is None and p.borrows == (kind == "borrow")
    return block


def _assert_borrowed(plan, rs, cs, batch, B, want, w_, y_):
    """A plan that borrows its pair fields: the six pointers of the struct it steps with are the epoch's arrays at the batch's
    position, and what lies there is what a plan with arrays of its own would hold."""
    st = plan.struct()
    off = 4 * batch * B
    for name, t in (("r_partner", rs.partner), ("r_w", rs.w), ("r_y", rs.y), ("c_partner", cs.partner), ("c_w", cs.w), ("c_y", cs.y)):
        assert getattr(st, name) == t.data_ptr() + off, name
    sl = slice(batch * B, (batch + 1) * B)
    np.testing.assert_array_equal(rs.partner[sl].cpu().numpy(), want["r_partner"])
    np.testing.assert_array_equal(cs.partner[sl].cpu().numpy(), want["c_partner"])
    np.testing.assert_array_equal(cs.w[sl].cpu().numpy(), w_[want["perm_r"]][want["c_perm"]])
    np.testing.assert_array_equal(cs.y[sl].cpu().numpy(), y_[want["perm_r"]][want["c_perm"]])


def _build_and_check(hip, plan_checker, rs, cs, block, runs, B, V, cap, kind, oracle):
    """build_plans_sorted of every (first batch, batches) of `runs` into poisoned plans: the device-side range check finds
    nothing and every plan equals oracle(batch)."""
    ws = _sorted_ws(hip, B, len(block))
    errors = torch.zeros(8, dtype=torch.int32, device=DEV)
    for first, count in runs:
        for p in block.plans:
            _poison(p, ws)
        hip.build_plans_sorted(rs, cs, first, block, count, V, ws)
        for j in range(count):
            b = first + j
            want, w_, y_ = oracle(b)
            assert (want["perm_r"] == np.arange(B)).all()    # the batch arrives sorted by row id
            plan = block.plans[j]
            plan_checker(plan, V, errors)
            _assert_plan_equals_oracle(plan, want, B, w_, y_)
            if kind == "borrow":
                _assert_borrowed(plan, rs, cs, b, B, want, w_, y_)
    assert errors.tolist() == [0] * 8, errors.tolist()


def _heavy_chunks():
    from trainer.hip_api import HEAVY_CHUNKS
    return HEAVY_CHUNKS


@functools.lru_cache(maxsize=None)
def _hand_oracle(row_runs, col_runs, cap, H):
    rs, _ = ec.hand_epoch(row_runs, col_runs)
    B = sum(row_runs)
    V = max(len(row_runs), len(col_runs)) + 2
    return tuple((ref.build_plan(rs[0][b * B:(b + 1) * B], rs[1][b * B:(b + 1) * B], cap, heavy_chunks=H, V=V),
                  rs[2][b * B:(b + 1) * B], rs[3][b * B:(b + 1) * B]) for b in range(ec.HAND_BATCHES))


HAND = [pytest.param(c, cap, id="%s-cap%d" % (c.label, cap)) for c in ec.hand_cases(_heavy_chunks()) for cap in c.caps]


@pytest.mark.parametrize("kind", ec.PLAN_KINDS)
@pytest.mark.parametrize("case,cap", HAND)
def test_sorted_build_of_hand_made_batches(hip, plan_checker, case, cap, kind):
    """Batches given by their run lengths on both sides — one pair, one id, all ids distinct, runs of 63 / 64 / 65 that end or
    start on a tile edge, runs over several tiles, runs of exactly heavy_chunks x cap pairs and one more — as three
    consecutive batches of an epoch, built from every first batch (batch starts take every residue), for the three kinds of
    staging plan."""
    H = _heavy_chunks()
    B, V = sum(case.row_runs), ec.hand_vocab(case)
    rs_np, cs_np = ec.hand_epoch(case.row_runs, case.col_runs)
    rs, cs = _pairs_from(rs_np), _pairs_from(cs_np)
    block = _block(hip, B, V, cap, kind, ec.HAND_BATCHES)
    assert block.plans[0].heavy_chunks == H                  # (the case table's H is the plans')
    oracle = _hand_oracle(case.row_runs, case.col_runs, cap, H)
    _build_and_check(hip, plan_checker, rs, cs, block, ec.HAND_RUNS, B, V, cap, kind, lambda b: oracle[b])


@functools.lru_cache(maxsize=None)
def _dealt_oracle(n, V, B, ids="uniform", V_row=0, seed=0, key=KEY, bad=False):
    """(stream, oracle masters, oracle epoch order of the row side) of a dealt epoch, shared by the tests on it."""
    if bad:
        stream = ec.fuzz_stream(dict(n=n, V=V, V_row=V_row, ids=ids, seed=seed, bad=True))
    else:
        stream = ec.masters_stream(n, V, V_row, ids, seed=seed)
    want_m = ref.build_masters(stream[0], stream[1], V, V_row or None)
    ir, ic = ref.deal_epoch(want_m, B, key)
    return stream, want_m, ir, ic


def _deal(hip, stream, V, B, key=KEY, V_row=0):
    n = len(stream[0])
    m = hip.build_masters(*_dev(*stream), V, V_row)
    rs, cs = _pairs(n, GUARD), _pairs(n, GUARD)
    _fill(rs, 0xFF); _fill(cs, 0xFF)
    ws = hip.deal_workspace(n, B, DEV)
    ws.fill_(0xFF)
    hip.deal_epoch(m, B, key, rs, cs, ws)
    return m, rs, cs


def _epoch_batch_oracle(want_m, ir, w, y, B, V, cap, H):
    @functools.lru_cache(maxsize=None)
    def oracle(b):
        idx = ir[b * B:(b + 1) * B]
        return ref.build_plan(want_m["row"][idx], want_m["col"][idx], cap, heavy_chunks=H, V=V), w[idx], y[idx]
    return oracle


@pytest.mark.parametrize("kind", ec.PLAN_KINDS)
@pytest.mark.parametrize("case", ec.SORTED_CASES, ids=label)
def test_sorted_build_behind_the_deal_small_and_odd_batches(hip, plan_checker, case, kind):
    """Masters, deal, then the index of every full batch: batches of one pair, below a wave, a wave +- 1, a tile +- 1, odd
    sizes (batch z starts at z B: no 16-byte alignment of anything), one id over three tiles in every batch, nearly all ids
    distinct at chunk cap 1."""
    n, V, B, cap = case.n, case.V, case.B, case.cap
    stream, want_m, ir, ic = _dealt_oracle(n, V, B)
    m, rs, cs = _deal(hip, stream, V, B)
    _assert_epoch(rs, cs, want_m, stream[2], stream[3], ir, ic, n)
    nb = n // B
    block = _block(hip, B, V, cap, kind, nb)
    oracle = _epoch_batch_oracle(want_m, ir, stream[2], stream[3], B, V, cap, block.plans[0].heavy_chunks)
    _build_and_check(hip, plan_checker, rs, cs, block, ((0, nb), (nb // 2, nb - nb // 2)), B, V, cap, kind, oracle)


# ---- steps on those plans ------------------------------------------------------------------------------------------------
_step_reference = {}


def _steps(hip, plans, V, d, B, form):
    from trainer.hip_api import DeviceTables, make_hyper
    t = DeviceTables(V, d, "Adagrad", seed=3)
    if form == 4:
        t.enable_twin()
    h = make_hyper(learning_rate=0.05, batch_size=B, step_form=form)
    loss = torch.zeros(4, device=DEV)
    losses = []
    for p in plans:
        hip.step_adagrad(p, t, h, loss)
        losses.append(loss.clone())
    out = {name: getattr(t, name).clone() for name in ("R", "C", "br", "bc")}
    out.update({"s1_" + name: t.s1[name].clone() for name in ("R", "C", "br", "bc")})
    out["loss"] = torch.stack(losses).view(torch.int32)
    return out


@pytest.mark.parametrize("kind,form", [(k, f) for k in ec.PLAN_KINDS for f in ec.STEP_FORMS[k]])
@pytest.mark.parametrize("B", ec.STEP_BATCH_SIZES)
def test_steps_on_small_and_odd_dealt_batches(hip, B, kind, form):
    """step_adagrad over all batches of an epoch on the staging plans == step_adagrad on glove_plan_build's plans of the same
    batches in the same arrival order, bit for bit: tables, Adagrad slots and loss words.  Borrowed plans (their pair-field
    pointers are not 16-byte aligned at odd B) therefore equal the run-word plans bit for bit, too."""
    V, d, cap = ec.STEP_V, ec.STEP_D, ec.STEP_CAP
    n = 5 * B + 3
    stream, _, _, _ = _dealt_oracle(n, V, B)
    m, rs, cs = _deal(hip, stream, V, B)
    nb = n // B
    block = _block(hip, B, V, cap, kind, nb)
    hip.build_plans_sorted(rs, cs, 0, block, nb, V, _sorted_ws(hip, B, nb))
    assert block.plans[0].fusable
    got = _steps(hip, block.plans, V, d, B, form)
    if (B, form) not in _step_reference:
        others = [hip.build_plan(*(t.contiguous() for t in rs.arrays(k * B, (k + 1) * B)), V, chunk_cap=cap, records=True, links=False,
                                 run_words=False) for k in range(nb)]
        assert others[0].r_crec is not None and others[0].r_chunk_hw is None
        _step_reference[(B, form)] = _steps(hip, others, V, d, B, form)
    want = _step_reference[(B, form)]
    for name in want:
        assert torch.equal(got[name].view(torch.int32), want[name].view(torch.int32)), name


# ---- fuzz ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("GLOVE_FUZZ_CASES", "24"))))
def test_randomized_dealt_epoch_is_bit_exact(hip, plan_checker, seed):
    """Seeded random (n, V, V_row, B, cap, id distribution, ids outside the tables, plan kind): masters, one deal and the sorted
    build of up to four batches from a random first one, all of it against the oracle."""
    c = ec.fuzz_case(seed)
    n, V, V_row, B, cap = c["n"], c["V"], c["V_row"], c["B"], c["cap"]
    stream, want_m, ir, ic = _dealt_oracle(n, V, B, c["ids"], V_row, c["seed"], c["key"], c["bad"])
    row, col, w, y = stream
    m, rs, cs = _deal(hip, stream, V, B, c["key"], V_row)
    assert m.mapped == ec.mapped_count(row, col, V, V_row)
    _assert_masters(m, want_m, w, y, n)
    _assert_epoch(rs, cs, want_m, w, y, ir, ic, n)
    assert _guards_intact(rs, cs)
    if not c["count"]:
        return
    block = _block(hip, B, V, cap, c["kind"], c["count"], V_row)
    oracle = _epoch_batch_oracle(want_m, ir, w, y, B, V, cap, block.plans[0].heavy_chunks)
    ws = _sorted_ws(hip, B, c["count"])
    errors = torch.zeros(8, dtype=torch.int32, device=DEV)
    for p in block.plans:
        _poison(p, ws)
    hip.build_plans_sorted(rs, cs, c["first"], block, c["count"], V, ws)
    for j in range(c["count"]):
        want, w_, y_ = oracle(c["first"] + j)
        plan_checker(block.plans[j], V, errors)
        _assert_plan_equals_oracle(block.plans[j], want, B, w_, y_)
        if c["kind"] == "borrow":
            _assert_borrowed(block.plans[j], rs, cs, c["first"] + j, B, want, w_, y_)
    assert errors.tolist() == [0] * 8, errors.tolist()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _null_field(pairs, field):
    """A glove_pairs struct like `pairs`' with one pointer NULL."""
    from trainer.hip_api import GlovePairs
    s = GlovePairs()
    for f in PAIR_FIELDS:
        setattr(s, f, None if f == field else getattr(pairs, f).data_ptr())
    return s


def test_masters_build_refuses(hip):
    """Every refusal returns its code before anything is launched: the poisoned outputs (the count of mapped ids among them)
    are as they were."""
    n, V = 100, 50
    row, col, w, y = _dev(*ec.masters_stream(n, V))
    rm, cm = _pairs(n), _pairs(n)
    link = torch.empty(n, dtype=torch.int32, device=DEV)
    mapped = torch.empty(1, dtype=torch.int32, device=DEV)
    size = hip.lib.glove_masters_workspace_bytes(n)
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    outputs = (link, mapped, ws)

    def poison():
        _fill(rm, 0xFF); _fill(cm, 0xFF)
        for t in outputs:
            t.view(torch.uint8).fill_(0xFF)

    def untouched():
        torch.cuda.synchronize()
        return _guards_intact_from0(rm, cm) and all(bool((t.view(torch.uint8) == 0xFF).all()) for t in outputs)

    def call(**kw):
        a = dict(row=row.data_ptr(), col=col.data_ptr(), w=w.data_ptr(), y=y.data_ptr(), n=n, V=V, V_row=0, rm=C.byref(rm.struct()),
                 cm=C.byref(cm.struct()), link=link.data_ptr(), mapped=mapped.data_ptr(), ws=ws.data_ptr(), ws_bytes=size)
        a.update(kw)
        poison()
        rc = hip.lib.glove_masters_build(a["row"], a["col"], a["w"], a["y"], a["n"], a["V"], a["V_row"], a["rm"], a["cm"], a["link"],
                                         a["mapped"], a["ws"], a["ws_bytes"], _stream())
        assert untouched(), kw
        return rc

    for kw in (dict(n=-1), dict(n=2 ** 31), dict(V=0), dict(V=-3), dict(V_row=-1), dict(V_row=V + 1)):
        assert call(**kw) == BADARG, kw
    for name in ("row", "col", "w", "y", "rm", "cm", "link", "ws"):
        assert call(**{name: None}) == BADARG, name
    for which in ("rm", "cm"):
        for f in PAIR_FIELDS:
            assert call(**{which: C.byref(_null_field(rm if which == "rm" else cm, f))}) == BADARG, (which, f)
    assert call(ws_bytes=size - 1) == WORKSPACE
    # and the same arguments unrefused build the masters
    poison()
    assert hip.lib.glove_masters_build(row.data_ptr(), col.data_ptr(), w.data_ptr(), y.data_ptr(), n, V, 0, C.byref(rm.struct()),
                                       C.byref(cm.struct()), link.data_ptr(), mapped.data_ptr(), ws.data_ptr(), size, _stream()) == 0
    assert mapped.item() == 0 and bool((rm.id[1:] >= rm.id[:-1]).all())


def _guards_intact_from0(*pairs):
    return all(bool((getattr(p, f).view(torch.uint8) == 0xFF).all()) for p in pairs for f in PAIR_FIELDS)


def test_epoch_deal_refuses(hip):
    n, V, B = 100, 50, 8
    m = hip.build_masters(*_dev(*ec.masters_stream(n, V)), V)
    rs, cs = _pairs(n), _pairs(n)
    size = hip.lib.glove_epoch_deal_workspace_bytes(n, B)
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    before = _snapshot(m.row_major, m.col_major, more=(m.link,))

    def call(**kw):
        a = dict(rm=C.byref(m.row_major.struct()), cm=C.byref(m.col_major.struct()), link=m.link.data_ptr(), n=n, B=B,
                 rs=C.byref(rs.struct()), cs=C.byref(cs.struct()), ws=ws.data_ptr(), ws_bytes=size)
        a.update(kw)
        _fill(rs, 0xFF); _fill(cs, 0xFF)
        ws.fill_(0xFF)
        rc = hip.lib.glove_epoch_deal(a["rm"], a["cm"], a["link"], a["n"], a["B"], KEY & (2 ** 64 - 1), KEY >> 64, a["rs"], a["cs"],
                                      a["ws"], a["ws_bytes"], _stream())
        torch.cuda.synchronize()
        assert _guards_intact_from0(rs, cs) and bool((ws == 0xFF).all()), kw
        assert _same(before, m.row_major, m.col_major, more=(m.link,)), kw
        return rc

    for kw in (dict(n=-1), dict(n=2 ** 31), dict(B=0), dict(B=-8)):
        assert call(**kw) == BADARG, kw
    assert call(rs=C.byref(m.row_major.struct())) == BADARG        # in place
    assert call(cs=C.byref(m.col_major.struct())) == BADARG
    for name in ("rm", "cm", "link", "rs", "cs", "ws"):
        assert call(**{name: None}) == BADARG, name
    for name, p in (("rm", m.row_major), ("cm", m.col_major), ("rs", rs), ("cs", cs)):
        for f in PAIR_FIELDS:
            assert call(**{name: C.byref(_null_field(p, f))}) == BADARG, (name, f)
    assert call(ws_bytes=size - 1) == WORKSPACE
    assert call(n=0) == 0
    hip.deal_epoch(m, B, KEY, rs, cs, ws)                   # and the same arguments unrefused deal an epoch
    assert bool((rs.id >= 0).all()) and bool((cs.id >= 0).all())


def test_epoch_deal_refuses_more_than_4m_batches(hip):
    """2^22 + 1 batches would need a digit of 12 bits: GLOVE_E_BADARG, nothing written (2^22 batches are dealt)."""
    n, B = ec.REFUSED_DEAL
    rm, cm, rs, cs = (_pairs(n) for _ in range(4))
    link = torch.zeros(n, dtype=torch.int32, device=DEV)
    size = max(hip.lib.glove_epoch_deal_workspace_bytes(n, B), 256)
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    for p in (rm, cm, rs, cs):
        _fill(p, 0xFF)
    ws.fill_(0xFF)
    rc = hip.lib.glove_epoch_deal(C.byref(rm.struct()), C.byref(cm.struct()), link.data_ptr(), n, B, 1, 2, C.byref(rs.struct()),
                                  C.byref(cs.struct()), ws.data_ptr(), size, _stream())
    torch.cuda.synchronize()
    assert rc == BADARG
    assert _guards_intact_from0(rs, cs) and bool((ws == 0xFF).all())


def _plan_bits(plan):
    names = PLAN_ARRAYS + ("r_crec", "c_crec", "r_mark", "c_mark", "r_chunk_hw", "c_chunk_hw")
    return [getattr(plan, n).view(torch.uint8).clone() for n in names if getattr(plan, n) is not None]


def test_plan_build_sorted_refuses(hip):
    from trainer.hip_api import GloveHipError, Plan, PlanBlock
    B, V, cap, nb = 100, 50, 4, 3
    stream, _, _, _ = _dealt_oracle(nb * B + 7, V, B)
    m, rs, cs = _deal(hip, stream, V, B)
    bound_u = min(B, V)
    bound_c = int(hip.lib.glove_plan_chunk_bound(B, bound_u, cap))
    size = hip.lib.glove_plan_sorted_workspace_bytes(B, nb)
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)

    def call(block, **kw):
        a = dict(rs=C.byref(rs.struct()), cs=C.byref(cs.struct()), first_pair=0, B=B, n=len(block), V=V, ws=ws.data_ptr(), ws_bytes=size)
        a.update(kw)
        for p in block.plans:
            _poison(p, ws)
        before = [_plan_bits(p) for p in block.plans]
        rc = hip.lib.glove_plan_build_sorted(a["rs"], a["cs"], a["first_pair"], a["B"], a["n"], a["V"], block.host, block.dev.data_ptr(),
                                             a["ws"], a["ws_bytes"], _stream())
        torch.cuda.synchronize()
        assert bool((ws == 0xFF).all()), kw
        for p, b in zip(block.plans, before):
            assert all(torch.equal(x, y) for x, y in zip(_plan_bits(p), b)), kw
        return rc

    good = _block(hip, B, V, cap, "records", nb)
    for kw in (dict(first_pair=-1), dict(B=0), dict(B=-B), dict(V=0), dict(V=-1), dict(n=-1)):
        assert call(good, **kw) == BADARG, kw
    assert call(good, B=B + 1) == BADARG                    # the plans' B is not the call's
    for name in ("rs", "cs", "ws"):
        assert call(good, **{name: None}) == BADARG, name
    for name, p in (("rs", rs), ("cs", cs)):
        for f in PAIR_FIELDS:
            assert call(good, **{name: C.byref(_null_field(p, f))}) == BADARG, (name, f)
    linked = PlanBlock([Plan(B, V, cap, DEV, cap_chunks=bound_c, cap_uniq=bound_u, records=True, links=True) for _ in range(nb)])
    assert linked.plans[0].c_perm is not None
    assert call(linked) == BADARG
    mixed = PlanBlock([hip.staging_plan(B, V, cap, DEV, **ec.plan_kind_args(k)) for k in ("records", "words", "records")])
    assert call(mixed) == BADARG
    other_B = PlanBlock([hip.staging_plan(B if j != 1 else B + 1, V, cap, DEV) for j in range(nb)])
    assert call(other_B) == BADARG
    few_ids = PlanBlock([Plan(B, V, cap, DEV, cap_chunks=bound_c, cap_uniq=bound_u - 1, records=True, links=False, own_pairs=False) for _ in range(nb)])
    assert call(few_ids) == WORKSPACE
    few_chunks = PlanBlock([Plan(B, V, cap, DEV, cap_chunks=bound_c - 1, cap_uniq=bound_u, records=True, links=False, own_pairs=False) for _ in range(nb)])
    assert call(few_chunks) == WORKSPACE
    assert call(good, ws_bytes=size - 1) == WORKSPACE
    assert call(good, n=0) == 0
    with pytest.raises(GloveHipError):
        hip.build_plans_sorted(rs, cs, 1, good, nb + 1, V, ws)         # more batches than the block holds
    with pytest.raises(GloveHipError):
        hip.build_plans_sorted(rs, cs, 1, good, nb, V, ws)             # batches 1 .. 3 of an epoch of 3 full batches
    # and the same block unrefused is built
    for p in good.plans:
        _poison(p, ws)
    hip.build_plans_sorted(rs, cs, 0, good, nb, V, ws)
    assert good.plans[nb - 1].counts.tolist()[1] > 0
