"""Every build of the two one-launch step kernels (tagged_step_kernel: Adagrad on step-tagged twins; tagged_adam_kernel: Adam on
twins flipped as a whole) at the smallest sizes that reach each branch of their shared chunk walk: one width per
(lanes per row, float4 per lane, exact fit) of glove_common.h pick_pass_shape, ids of more chunks than plan.heavy_chunks, trips of
U - 1 / U / U + 1 pairs for both unrolls, a full record and a second chunk of one pair, both heads, and chains whose steps find a
record left by a launch with another row-side grid.

Asserted as in test_gpu_onestep.py / test_gpu_onestep_adam.py, whose tolerances these are: the float64 oracle
(loss rtol 1e-5, parameters and slots rtol 1e-5 / atol 1e-6; 2e-5 / 2e-6 after Adam's third step), the form really ran, and bit
equality with the two-launch form on every untouched or swept row and every id of up to heavy_chunks chunks.

That bit equality is a property of ONE step from equal tables.  Adam's three steps are therefore each compared with a two-launch
step that starts from the state the one-launch run was in (_adam_single_steps): carried over three steps of two separate runs it
does not hold, in any build — the heavy id's row, and the global bias once an id has several chunks, differ in the last bit
after the first step, and the ids paired with them inherit that (V = 128, B = 120, chunk_cap 4, one id of 10 chunks: after the
third step one element of m of a col id of one pair, relative 6.5e-8 at d = 512, at 7 of the 16 widths)."""
import numpy as np
import pytest
import torch

import glove_ref as ref
from helpers import _mid_run, _tagged, _twinned, assert_tables_close, make_batch, oracle_tables, tables_from_oracle, to_dev

pytestmark = pytest.mark.gpu

B, V = 120, 128                             # Adam's one-launch form needs 2 B <= V_row + V
FULL_WIDTHS = (32, 64, 128, 256, 384, 512, 768, 1024)
PART_WIDTHS = (20, 52, 100, 200, 300, 400, 600, 900)
# (lanes per row, float4 per lane, lanes x float4 == float4 per row) each width must select
SHAPES = {32: (8, 1, True), 64: (8, 2, True), 128: (32, 1, True), 256: (64, 1, True), 384: (32, 3, True), 512: (64, 2, True),
          768: (64, 3, True), 1024: (64, 4, True), 20: (8, 1, False), 52: (8, 2, False), 100: (32, 1, False), 200: (64, 1, False),
          300: (32, 3, False), 400: (64, 2, False), 600: (64, 3, False), 900: (64, 4, False)}
TRIP_LENGTHS = (1, 3, 4, 5, 7, 8, 9, 32, 33)


def _pass_shape(d4):
    """glove_common.h pick_pass_shape, restated: 8 lanes up to 16 float4 per row, then the candidate with the fewest slots that
    hold the row (the first listed wins a tie)."""
    if d4 <= 8:
        return 8, 1
    if d4 <= 16:
        return 8, 2
    best = None
    for lpr, nv in ((16, 1), (32, 1), (64, 1), (32, 3), (64, 2), (64, 3), (64, 4)):
        if lpr * nv >= d4 and (best is None or lpr * nv < best[0] * best[1]):
            best = (lpr, nv)
    return best


def _shape_of(tables):
    d4 = tables.d // 4
    lpr, nv = _pass_shape(d4)
    return lpr, nv, lpr * nv == d4


def test_every_build_has_a_width():
    assert sorted(SHAPES) == sorted(FULL_WIDTHS + PART_WIDTHS)
    got = {_pass_shape((d + 3) // 4) + (_pass_shape((d + 3) // 4)[0] * _pass_shape((d + 3) // 4)[1] == (d + 3) // 4,) for d in SHAPES}
    want = {(lpr, nv, full) for lpr, nv in ((8, 1), (8, 2), (32, 1), (32, 3), (64, 1), (64, 2), (64, 3), (64, 4)) for full in (False, True)}
    assert got == want and all(SHAPES[d][2] == (d in FULL_WIDTHS) for d in SHAPES)


def _hyper(hp, form):
    from trainer.hip_api import make_hyper
    return make_hyper(l2_reg=hp.l2_reg, reg_mult=hp.reg_mult, learning_rate=hp.learning_rate, epsilon=hp.epsilon, batch_size=B,
                      head=hp.head, neg_factor=hp.neg_factor, step_form=form)


def _skewed_batch(d, head=0):
    """Case A's batch: one id with at least 40 pairs — 10 chunks at chunk_cap 4, more than plan.heavy_chunks."""
    row, col, w, y = make_batch(B + V + d, B, V)
    row[::3] = 3
    if head == 1:
        y = np.abs(y) * 0.1
    return row, col, w, y


def _trip_edge_batch(d):
    """Case B's batch: row ids of exactly 1, 3, 4, 5, 7, 8, 9, 32 and 33 pairs and col ids likewise, the rest of the B pairs on ids
    that occur once (row ids 0 .. 26, col ids 40 .. 66: never equal)."""
    _, _, w, y = make_batch(B + V + d, B, V)
    lengths = np.array(TRIP_LENGTHS + (1,) * (B - sum(TRIP_LENGTHS)))
    row = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    col = (40 + np.repeat(np.arange(len(lengths)), lengths)).astype(np.int32)
    col = col[np.random.default_rng(d).permutation(B)]
    for ids in (row, col):
        counts = np.bincount(ids)
        assert set(TRIP_LENGTHS) <= set(counts.tolist()) and counts.max() == 33 and len(ids) == B
    return row, col, w, y


def _same_as_two_launch_form(a, b, want, plan, slots, swept):
    """Bit equality of tables a (one launch) and b (two launches): on every id of up to heavy_chunks chunks, and on every row no
    id of the batch names — all of them if the form sweeps the tables (Adam), which then covers the slots of the biases too."""
    for side, name, bias in (("r", "R", "br"), ("c", "C", "bc")):
        rec = want[side + "_uniq_rec"]
        same = torch.ones(V, dtype=torch.bool, device="cuda:0")
        same[torch.from_numpy(rec[rec[:, 2] > plan.heavy_chunks, 0].astype(np.int64)).cuda()] = False
        if not swept:
            one = torch.from_numpy(rec[rec[:, 2] <= plan.heavy_chunks, 0].astype(np.int64)).cuda()
            for s in slots:
                assert torch.equal(s(a)[name][one], s(b)[name][one]), name
        assert torch.equal(getattr(a, name)[same], getattr(b, name)[same]), name
        assert torch.equal(getattr(a, bias)[same], getattr(b, bias)[same]), bias
        if swept:
            for s in slots:
                assert torch.equal(s(a)[name][same], s(b)[name][same]), name
                assert torch.equal(s(a)[bias][same], s(b)[bias][same]), bias


def _close_to_two_launch_form(la, lb, a, b, want):
    if int(want["r_uniq_rec"][:, 2].max()) == 1:        # every row id in one chunk: the loss partials add up in the same order
        np.testing.assert_array_equal(la.cpu().numpy(), lb.cpu().numpy())
        assert torch.equal(a.scalars, b.scalars)
    np.testing.assert_allclose(la.cpu().numpy(), lb.cpu().numpy(), rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(a.scalars.cpu().numpy(), b.scalars.cpu().numpy(), rtol=2e-6, atol=1e-9)


def _adagrad_single_step(hip, d, batch, cap, head=0):
    """test_one_launch_single_step's assertions."""
    from trainer.hip_api import DeviceTables
    hp = ref.Hyper(learning_rate=0.05, head=head, neg_factor=0.7)
    row, col, w, y = batch
    t = oracle_tables(V, d, "Adagrad")
    a, b = _tagged(t), tables_from_oracle(t, DeviceTables)
    assert _shape_of(a) == SHAPES[d]
    plan = hip.build_plan(*to_dev(row, col, w, y), V, chunk_cap=cap, records=True)
    la, lb = torch.zeros(4, device="cuda:0"), torch.zeros(4, device="cuda:0")
    hip.step_adagrad(plan, a, _hyper(hp, 5), la)
    assert int((a.R_tag != 0).sum()) == int(plan.counts[1]) and int((a.C_tag != 0).sum()) == int(plan.counts[3])    # the form really ran
    hip.step_adagrad(plan, b, _hyper(hp, 1), lb)
    loss, L, reg = ref.train_step(t, row, col, w, y, hp)
    np.testing.assert_allclose(la.cpu().numpy()[:3], [loss, L, reg], rtol=1e-5)
    assert_tables_close(a, t, 1e-5, 1e-6)
    want = ref.build_plan(row, col, cap, V=V)
    _close_to_two_launch_form(la, lb, a, b, want)
    assert a.global_step == b.global_step == 1
    _same_as_two_launch_form(a, b, want, plan, (lambda x: x.s1,), swept=False)
    return want


def _plain_copy(s):
    """Plain tables holding the state of s (reading s brings its rows home)."""
    from trainer.hip_api import DeviceTables
    b = DeviceTables(s.V, s.d_model, s.optimizer, device="cuda:0", seed=0)
    for n in ("R", "C", "br", "bc"):
        getattr(b, n).copy_(getattr(s, n))
        b.s1[n].copy_(s.s1[n])
        b.s2[n].copy_(s.s2[n])
    b.scalars.copy_(s.scalars)
    b.step.copy_(s.step)
    return b


def _adam_single_steps(hip, d, batch, cap, head=0):
    """test_one_launch_adam_single_steps' assertions: two steps (the second reads the second copies) and a third one, never read
    in between, against the oracle; and each of the three steps against a two-launch step from the same state (the module's
    docstring) — the state the one-launch run is in before and after step k + 1 comes from runs of their own, k and k + 1
    steps long, because reading tables brings their rows home."""
    hp = ref.Hyper(learning_rate=0.001, head=head, neg_factor=0.7)
    row, col, w, y = batch
    t = _mid_run(V, d)
    a = _twinned(t)
    assert _shape_of(a) == SHAPES[d]
    plan = hip.build_plan(*to_dev(row, col, w, y), V, chunk_cap=cap, records=True)
    assert plan.r_mark is not None
    want = ref.build_plan(row, col, cap, V=V)
    Ga, Gb, Gs = (hip.dense_grad_buffer(a) for _ in range(3))
    la, lb, ls = (torch.zeros(4, device="cuda:0") for _ in range(3))

    def run_of(steps):
        s = _twinned(_mid_run(V, d))
        for _ in range(steps):
            hip.step_adam(plan, s, _hyper(hp, 0), Gs, ls)
        return s

    for k in range(3):
        hip.step_adam(plan, a, _hyper(hp, 0), Ga, la)
        assert float(a.scalars[3]) == float((k + 1) % 2) and a._twin_dirty          # the form really ran: the tables flipped
        loss, L, reg = ref.train_step(t, row, col, w, y, hp)
        if k < 2:
            np.testing.assert_allclose(la.cpu().numpy()[:3], [loss, L, reg], rtol=1e-5)
        b = _plain_copy(run_of(k))
        hip.step_adam(plan, b, _hyper(hp, 1), Gb, lb)
        after = run_of(k + 1)
        assert float(after.scalars[3]) == float((k + 1) % 2)
        _same_as_two_launch_form(after, b, want, plan, (lambda x: x.s1, lambda x: x.s2), swept=True)
        _close_to_two_launch_form(ls, lb, after, b, want)
        assert after.global_step == b.global_step == 17 + k + 1
    assert float(a.scalars[3]) == 1.0
    assert_tables_close(a, t, 2e-5, 2e-6)                                             # (reading brings the rows home)
    assert float(a.scalars[3]) == 0.0 and int((a.R_tag != 0).sum()) == 0
    assert float(Ga.abs().max()) == 0.0 and float(Gs.abs().max()) == 0.0
    assert a.global_step == 20
    for n in ("R", "C", "br", "bc"):                                                  # the runs of their own are this run
        assert torch.equal(getattr(a, n), getattr(after, n)) and torch.equal(a.s1[n], after.s1[n]) and torch.equal(a.s2[n], after.s2[n]), n
    assert torch.equal(a.scalars, after.scalars) and torch.equal(la, ls)
    return want


SINGLE = {"Adagrad": _adagrad_single_step, "Adam": _adam_single_steps}


@pytest.mark.parametrize("optimizer", ["Adagrad", "Adam"])
@pytest.mark.parametrize("d", FULL_WIDTHS + PART_WIDTHS)
def test_a_single_steps_at_every_build(hip, d, optimizer):
    """Every (shape, exact fit) of both kernels on a batch with an id of 10 chunks at chunk_cap 4."""
    want = SINGLE[optimizer](hip, d, _skewed_batch(d), 4)
    assert int(want["r_uniq_rec"][:, 2].max()) >= 10 > 8                             # (8: plan.heavy_chunks)


@pytest.mark.parametrize("optimizer", ["Adagrad", "Adam"])
@pytest.mark.parametrize("d", [32, 64, 300, 1024])
def test_b_trip_edges(hip, d, optimizer):
    """Ids of U - 1, U and U + 1 pairs for the unrolls 8 (one float4 per lane: d = 32) and 4, a record of all 32 pairs and a
    second chunk of one pair, at chunk_cap 32."""
    want = SINGLE[optimizer](hip, d, _trip_edge_batch(d), 32)
    for side in ("r", "c"):
        rec = want[side + "_uniq_rec"]                                               # {id, first chunk, chunks, pairs}
        assert set(TRIP_LENGTHS) <= set(rec[:, 3].tolist()) and sorted(rec[rec[:, 3] >= 32, 2].tolist()) == [1, 2]


@pytest.mark.parametrize("optimizer", ["Adagrad", "Adam"])
@pytest.mark.parametrize("d", [52, 256, 600])
def test_c_logistic_head(hip, d, optimizer):
    """head = 1 (logistic matrix factorisation, neg_factor 0.7, counts |y| / 10) on case A's batch."""
    SINGLE[optimizer](hip, d, _skewed_batch(d, head=1), 4, head=1)


@pytest.mark.parametrize("optimizer", ["Adagrad", "Adam"])
@pytest.mark.parametrize("d", [64, 200, 768])
def test_d_chains(hip, d, optimizer):
    """Three steps on plans of chunk_cap 4, 32 and 4 as one chain, as chains of two and one (a workspace of two chain records)
    and one by one: the same bits.  Each step of a chain derives its global bias from a record whose partials a launch with
    another row-side grid left (the grid follows plan.cap_chunks)."""
    adam = optimizer == "Adam"
    hp = ref.Hyper(learning_rate=0.01 if adam else 0.05)
    t = _mid_run(V, d, seed=9, step=3) if adam else oracle_tables(V, d, "Adagrad")
    a, b, c = ((_twinned if adam else _tagged)(t) for _ in range(3))
    # (ids drawn evenly at chunk_cap 4, Zipf ids at 32: about 80 and 50 chunks, another number of workgroups at every shape)
    plans = [hip.build_plan(*to_dev(*make_batch(80 + k, B, V, zipf=cap == 32)), V, chunk_cap=cap, records=True).compact(hip.lib, records=True)
             for k, cap in enumerate((4, 32, 4))]
    assert plans[0].cap_chunks != plans[1].cap_chunks != plans[2].cap_chunks
    groups = 256 // SHAPES[d][0]                                                    # lane groups (= chunks in flight) per workgroup
    blocks = [-(-p.cap_chunks // groups) for p in plans]
    assert blocks[0] != blocks[1] != blocks[2]
    h = _hyper(hp, 5)
    G = hip.dense_grad_buffer(a) if adam else None
    la, lb, lc = (torch.zeros(4, device="cuda:0") for _ in range(3))
    full = torch.empty(max(hip.lib.glove_step_workspace_bytes(B, p.cap_chunks, a.d) for p in plans), dtype=torch.uint8, device="cuda:0")
    two = torch.empty(2 * (8 + 4 * max(blocks)) * 4, dtype=torch.uint8, device="cuda:0")       # a record: 8 floats + 4 per row-side workgroup
    hip.steps(plans, a, h, G, la, full)
    hip.steps(plans, b, h, G, lb, two)
    for p in plans:
        hip.step(p, c, h, G, lc, full)
    first = t.step
    assert a.global_step == b.global_step == c.global_step == first + 3
    if adam:
        assert float(a.scalars[3]) == float(b.scalars[3]) == float(c.scalars[3]) == 1.0     # three flips
    assert torch.equal(la, lb) and torch.equal(la, lc)                                       # the LAST step's loss
    assert torch.equal(a.scalars, b.scalars) and torch.equal(a.scalars, c.scalars)
    for n in ("R", "C", "br", "bc"):
        for x in (b, c):
            assert torch.equal(getattr(a, n), getattr(x, n)), n
            assert torch.equal(a.s1[n], x.s1[n]), n
            if adam:
                assert torch.equal(a.s2[n], x.s2[n]), n
