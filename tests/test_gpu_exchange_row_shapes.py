"""The kernels of the touched-rows and dense exchange of the multi-GPU forms at every row shape (csrc/glove_step.hip:
count_packed_kernel, combine_packed_kernel <LPR, NV>, decay_unmarked_kernel <LPR, NV, OPT>, apply_packed_kernel <LPR, NV, OPT>,
gather_rows_kernel <LPR, NV>, dense_grad_kernel <LPR, NV>, pack_grad_kernel <LPR, NV>), on the exact lists of
tests/exchange_shape_cases.py; tests/test_exchange_shape_cases.py proves on the references alone what is relied on here.

  - the fifteen tables of tests/row_shape_cases.py — the first and the last width of each of the seven shapes, and 257 model
    columns on a stride of 260 — times six lists of several ranks (three bare ones, one with a header under a capacity above
    its count, one with the `ids` and `side` overrides, an empty one) whose ids are named by one list, by two to four
    (the first of them not always list 0) and by none: a later list adds behind a first store, an id one list names skips
    the dense buffer behind count_packed, and todo 0 / 1 / 2 mix inside the lane groups of apply_packed_kernel.  The dense
    buffer (pre-filled with NaN) and the marks are compared for EQUALITY with float64, the applied tables of Adagrad, Adam,
    RMSprop and Adamax at the project's rtol 1e-5 / atol 1e-6 (one float4 lost from a sum misses it 389-fold at least under
    Adagrad); rows no list names and the side hyper.sides leaves out keep their bits.  Eleven lists with tail = NULL.
  - four lists longer than one grid sweep at one width of every lanes-per-row count (3T + 2, 2T + 1, 2T and T entries for
    the T lane groups of a full grid): lane groups of one to four entries, pairs whose second entry is past the end, the
    grid-stride loop of combine_packed_kernel and, under Adam, the kSweepRows stride of decay_unmarked_kernel.

The tests elsewhere (test_gpu_parity.py, test_gpu_sharded_optimizers.py) run several lists at three of the seven shapes and
long lists at LPR 32 only; test_gpu_optimizer_matrix.py reaches all seven with one list of one rank."""
import os

import numpy as np
import pytest
import torch

import exchange_shape_cases as xc
import glove_ref as ref
import row_shape_cases as rc
from helpers import assert_opt_tables_close, opt_tables_from_oracle, to_dev
from sharded_oracle_backend import restricted_update

pytestmark = pytest.mark.gpu
TABLE_IDS = ["d%d_stride%d" % t for t in xc.TABLES]
F64 = np.float64
NAN = float("nan")


def tables_at(t, stride):
    """Device tables of the oracle's state on a row stride of the test's choosing: d rounded up to whole float4, the rule
    GLOVE_ROW_ALIGN=4 selects (DeviceTables would otherwise move some widths onto a 64-byte stride and another kernel shape)."""
    from trainer.hip_api import DeviceTables
    old = os.environ.get("GLOVE_ROW_ALIGN")
    os.environ["GLOVE_ROW_ALIGN"] = "4"
    try:
        dt = opt_tables_from_oracle(t, DeviceTables)
    finally:
        if old is None:
            del os.environ["GLOVE_ROW_ALIGN"]
        else:
            os.environ["GLOVE_ROW_ALIGN"] = old
    assert dt.d == stride and dt.d_model == t.d and dt.V_row == dt.V == t.V
    return dt


def upload(hip, c):
    """(the glove_packed_list of every list of the case, the device buffers they point into)."""
    packed, keep = [], []
    for l in c.lists:
        n = len(l["ids"])
        if l["kind"] == "header":
            # behind the count, up to the capacity: entries no kernel may read (they name row id 0: reading them would show)
            rest = np.full((c.capacity - n, c.stride + 4), 5.0, np.float32)
            rest[:, c.stride + 1:] = 0.0
            buf, = to_dev(np.concatenate([xc.header_of(l, c.stride), l["entries"], rest]))
            packed.append(hip.packed_list(buf))
        else:
            buf, = to_dev(l["entries"] if n else np.zeros((1, c.stride + 4), np.float32))
            ids = to_dev(l["ids"])[0] if l["kind"] == "override" else None
            packed.append(hip.packed_list(buf, with_header=False, ids=ids, n=n, side=l["fixed_side"]))
            keep.append(ids)
        keep.append(buf)
    return packed, keep


def nan_buffer(hip, dt):
    """A dense gradient buffer whose rows and biases hold NaN (a first touch stores, it does not add); the tail stays zero."""
    G = hip.dense_grad_buffer(dt)
    G[:hip.grad_layout(dt)["tail"]] = NAN
    return G


def views(hip, dt, G):
    """([G_R, G_C] as [V, stride], [G_br, G_bc]) of a dense gradient buffer."""
    lay = hip.grad_layout(dt)
    rows = [G[lay[n]:lay[n] + dt.V * dt.d].view(dt.V, dt.d) for n in ("G_R", "G_C")]
    return rows, [G[lay[n]:lay[n] + dt.V] for n in ("G_br", "G_bc")]


def assert_dense_buffer(hip, dt, G, want, counted):
    """The rows and biases of the ids several lists name EQUAL the float64 sums; of the ids one list names too where nothing
    was counted, otherwise they were never written; nor were those of the ids no list names."""
    Gw, Gbw, count, _ = want
    rows, biases = views(hip, dt, G)
    for s in (0, 1):
        for got, w in ((rows[s], Gw[s]), (biases[s], Gbw[s])):
            w32 = torch.from_numpy(w.astype(np.float32)).cuda()
            assert (w.astype(np.float32).astype(F64) == w).all()
            for k, written in ((0, False), (1, not counted), (2, True)):
                sel = torch.from_numpy(count[s] == k if k < 2 else count[s] >= 2).cuda()
                assert bool(sel.any()) or not count[s].any()
                if written:
                    wrong = (got[sel] != w32[sel]).nonzero()
                    assert wrong.numel() == 0, ("side %d, ids named by %d lists: first wrong (id, column)" % (s, k), wrong[:8].tolist())
                else:
                    assert bool(torch.isnan(got[sel]).all()), "side %d: an id named by %d lists was written" % (s, k)


@pytest.mark.parametrize("counted", [False, True], ids=["combine", "count+combine"])
@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_count_and_combine_equal_float64(hip, dm, stride, counted):
    c = xc.case(dm, stride, 3, 6)
    print("d_model %d stride %d: shape (lpr, nv) = %s, lists of %s entries, capacity %d"
          % (dm, stride, xc.pick_row_shape(stride // 4), [len(l["ids"]) for l in c.lists], c.capacity))
    dt = tables_at(xc.seeded_tables(c.V, dm, "Adagrad"), stride)
    packed, keep = upload(hip, c)
    G = nan_buffer(hip, dt)
    mark = torch.zeros(2 * c.V, dtype=torch.int32, device="cuda:0")
    if counted:
        hip.count_packed(packed, dt, G, mark, c.capacity)
    for k, lst in enumerate(packed):
        hip.combine_packed(lst, k, dt, G, mark, c.capacity)
    torch.cuda.synchronize()
    want = xc.dense_reference(c)
    assert_dense_buffer(hip, dt, G, want, counted)
    np.testing.assert_array_equal(mark.cpu().numpy().reshape(2, c.V), xc.mark_words(want[2], want[3], counted))


def state_of(dt):
    out = {n: getattr(dt, n).clone() for n in ("R", "C", "br", "bc")}
    for k, slot in (("s1", dt.s1), ("s2", dt.s2)):
        out.update({k + n: x.clone() for n, x in slot.items()})
    return out


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_exchange(hip, c, packed, optimizer, sides, counted, tail, want):
    """count (optional) + the combines in list order + the apply on fresh tables of `optimizer`, against the float64 oracle:
    every variable and slot at the project's tolerance, the marks zero again, the bits that must not move."""
    from trainer.hip_api import make_hyper
    Gw, Gbw, count, first = want
    t = xc.seeded_tables(c.V, c.dm, optimizer)
    dt = tables_at(t, c.stride)
    dt.step.fill_(xc.STEP + 1)                               # as this step's row pass leaves it
    before, scalars_before = state_of(dt), dt.scalars.clone()
    G = nan_buffer(hip, dt)
    mark = torch.zeros(2 * c.V, dtype=torch.int32, device="cuda:0")
    hp = ref.Hyper(learning_rate=xc.LR[optimizer])
    h = make_hyper(learning_rate=hp.learning_rate, batch_size=4096, sides=sides, optimizer=optimizer)
    loss_out = torch.zeros(4, device="cuda:0")
    if counted:
        hip.count_packed(packed, dt, G, mark, c.capacity)
    for k, lst in enumerate(packed):
        hip.combine_packed(lst, k, dt, G, mark, c.capacity)
    assert_dense_buffer(hip, dt, G, want, counted)
    tail_t = torch.tensor(tail, device="cuda:0") if tail is not None and sides & 2 else None
    hip.apply_packed(packed, dt, h, G, mark, tail_t, loss_out, c.capacity)
    torch.cuda.synchronize()
    # without a tail the apply sums the loss partials of the lists' headers, in list order (multiples of 1/8: exact)
    sum_e = tail[0] if tail is not None else sum(float(l["partials"][0]) for l in c.lists if l["kind"] == "header")
    restricted_update(t, xc.gradients_of(c, Gw, Gbw, count, sum_e), hp, sides)
    if not sides & 2:                    # no scalar work: the global bias and its slots untouched, global_step as the pass left it
        t.step = xc.STEP + 1
        assert same_bits(dt.scalars, scalars_before)
    assert_opt_tables_close(dt, t, xc.RTOL, xc.ATOL)
    assert int(mark.abs().sum()) == 0, "marks left behind"
    assert float(G[hip.grad_layout(dt)["tail"]:].abs().max()) == 0.0, "the tail of the dense buffer is not zero again"
    after = state_of(dt)
    for s, bit, names in ((0, 1, ("R", "br")), (1, 2, ("C", "bc"))):
        keys = [k + n for n in names for k in ("", "s1", "s2") if k + n in after]
        unnamed = torch.from_numpy(count[s] == 0).cuda()
        assert bool(unnamed.any())
        for key in keys:
            if not sides & bit:
                assert same_bits(after[key], before[key]), key + " of the side left out moved"
            elif optimizer in ("Adagrad", "Adamax"):         # only touched rows move
                assert same_bits(after[key][unnamed], before[key][unnamed]), key + ": a row no list names moved"
            elif key.startswith("s1"):                       # Adam, RMSprop: the G = 0 update decays every unnamed row's slot
                a, b = (x[key][unnamed][:, :c.dm] if x[key].dim() == 2 else x[key][unnamed] for x in (after, before))
                assert bool((a != b).all()), key + ": a row no list names was not swept"
    return dt


@pytest.mark.parametrize("sides", [1, 2, 3])
@pytest.mark.parametrize("optimizer", xc.OPTIMIZERS)
@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_apply_packed_matches_float64(hip, dm, stride, optimizer, sides):
    c = xc.case(dm, stride, sides, 6)
    packed, keep = upload(hip, c)
    run_exchange(hip, c, packed, optimizer, sides, True, xc.TAIL, xc.dense_reference(c))


@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_apply_packed_of_eleven_lists_without_a_tail(hip, dm, stride):
    """Two launches of the apply (eight lists and three), the loss partials summed over ALL headers first, nothing counted:
    every named id comes out of the dense buffer, from the list that stored it first."""
    c = xc.case(dm, stride, 3, 11)
    packed, keep = upload(hip, c)
    run_exchange(hip, c, packed, "Adagrad", 3, False, None, xc.dense_reference(c))


@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_gather_rows_equals_the_table(hip, dm, stride):
    R, _, br, _, _ = rc.eval_tables(dm, stride)
    V, n = R.shape[0], 1003                                  # no multiple of a block's 4, 8 or 16 lane groups
    rng = np.random.default_rng(dm)
    ids = rng.integers(0, V, n).astype(np.int32)             # random order, repeats
    ids[:4] = (0, V - 1, V - 1, 0)
    assert n % 4 and len(np.unique(ids)) < n
    W, bias, ids_t = to_dev(R, br.astype(np.float32), ids)
    rows = torch.full((n, stride), NAN, device="cuda:0")
    biases = torch.full((n,), NAN, device="cuda:0")
    hip.gather_rows(W, bias, ids_t, rows, biases)
    torch.cuda.synchronize()
    assert torch.equal(rows, W[ids_t.long()]) and torch.equal(biases, bias[ids_t.long()])


@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_dense_grad_and_pack_grad_agree_bit_for_bit(hip, dm, stride):
    """The plan's summed gradients as a dense buffer (dense_grad_kernel) and as a packed list (pack_grad_kernel) on the exact
    step tables of tests/row_shape_cases.py, B = 1,024 pairs in chunks of two and no L2 term: the list combined alone IS the dense buffer, bit
    for bit; both match glove_ref.gradients at the tolerance tests/test_gpu_parity.py holds the per-pair e to (rtol 1e-5,
    atol 1e-7); the header counts, the id order and the sides are the plan's."""
    from trainer.hip_api import make_hyper
    B = 1024
    R, C_, br, bc, g = rc.eval_tables(dm, stride)
    V = R.shape[0]
    row, col, w, y = rc.eval_batch(B)
    t = ref.Tables(V, dm, "Adagrad", dtype=np.float32, seed=1).astype(F64)
    t.R, t.C, t.br, t.bc, t.g = R[:, :dm].astype(F64), C_[:, :dm].astype(F64), br.astype(F64), bc.astype(F64), F64(g)
    dt = tables_at(t, stride)
    hp = ref.Hyper(learning_rate=0.05, l2_reg=0.0)
    h = make_hyper(learning_rate=0.05, batch_size=B, l2_reg=0.0)
    plan = hip.build_plan(*to_dev(row, col, w, y), V, chunk_cap=2, compact=True)
    ur, uc = np.unique(row), np.unique(col)
    n_r, n_c = plan.host_counts[1], plan.host_counts[3]
    assert (n_r, n_c) == (len(ur), len(uc))
    G = hip.dense_grad_buffer(dt)
    packed = torch.full((1 + n_r + n_c + 3, stride + 4), NAN, device="cuda:0")
    hip.passes(plan, dt, h)
    hip.dense_grad(plan, dt, h, G)
    hip.pack_grad(plan, dt, h, packed)
    G2 = nan_buffer(hip, dt)
    mark = torch.zeros(2 * V, dtype=torch.int32, device="cuda:0")
    hip.combine_packed(hip.packed_list(packed), 0, dt, G2, mark, packed.shape[0])
    torch.cuda.synchronize()
    # the header, the ids in plan order (ascending, the row side first), the sides; nothing behind the last entry
    assert packed[0, :2].view(torch.int32).tolist() == [n_r, n_c]
    body = packed[1:1 + n_r + n_c]
    np.testing.assert_array_equal(body[:, stride + 1].view(torch.int32).cpu().numpy(), np.r_[ur, uc])
    np.testing.assert_array_equal(body[:, stride + 2].view(torch.int32).cpu().numpy(), np.r_[np.zeros(n_r, int), np.ones(n_c, int)])
    assert bool(torch.isnan(packed[1 + n_r + n_c:]).all()) and not bool(torch.isnan(body).any())
    (rows, biases), (rows2, biases2) = views(hip, dt, G), views(hip, dt, G2)
    gr = ref.gradients(t, row, col, w, y, hp)
    for s, named, GW, Gb in ((0, ur, "G_R", "G_br"), (1, uc, "G_C", "G_bc")):
        sel = torch.zeros(V, dtype=torch.bool, device="cuda:0")
        sel[torch.from_numpy(named).cuda().long()] = True
        assert torch.equal(rows2[s][sel], rows[s][sel]) and torch.equal(biases2[s][sel], biases[s][sel])
        assert bool(torch.isnan(rows2[s][~sel]).all()) and bool(torch.isnan(biases2[s][~sel]).all())
        assert bool((~sel).any()) and float(rows[s][~sel].abs().max()) == 0.0
        assert stride == dm or float(rows[s][:, dm:].abs().max()) == 0.0
        np.testing.assert_allclose(rows[s][:, :dm].cpu().numpy(), gr[GW], rtol=1e-5, atol=1e-7, err_msg=GW)
        np.testing.assert_allclose(biases[s].cpu().numpy(), gr[Gb], rtol=1e-5, atol=1e-7, err_msg=Gb)
        assert (gr[GW][named] != 0).mean() > 0.9
    np.testing.assert_array_equal(mark.cpu().numpy().reshape(2, V), np.stack([np.isin(np.arange(V), x) for x in (ur, uc)]).astype(np.int32) << 8)


LONG_CASES = [(d, "Adagrad") for d in sorted(xc.LONG_WIDTHS.values())] + [(d, "Adam") for d in xc.LONG_ADAM]


@pytest.mark.parametrize("stride,optimizer", LONG_CASES)
def test_lists_longer_than_one_grid_sweep(hip, stride, optimizer):
    """3T + 2, 2T + 1, 2T and T entries for the T lane groups of a full grid: apply_packed_kernel's groups hold one to four
    entries (two pairs, the second entry of a pair past the end), combine_packed_kernel strides its grid, and under Adam
    (LPR 16 and LPR 64) decay_unmarked_kernel strides over more than kSweepRows rows per group."""
    c = xc.long_case(stride)
    lpr, nv = xc.pick_row_shape(stride // 4)
    print("stride %d: shape (%d, %d), T = %d lane groups, lists of %s entries, %d ids a side"
          % (stride, lpr, nv, xc.lane_groups(stride), [len(l["ids"]) for l in c.lists], c.V))
    packed, keep = upload(hip, c)
    run_exchange(hip, c, packed, optimizer, 3, True, xc.TAIL, xc.dense_reference(c))
