"""The cases of tests/test_gpu_exchange_row_shapes.py, proved on the references alone (no GPU): the widths reach every row
shape twice, the lists hold what the GPU tests mean to exercise (every kind of list, ids named by one, by several and by no
list on both sides, a first namer other than list 0), every sum over lists is exact in float32 in either list order, the long
lists give lane groups of one, two, three and four entries and a pair whose second entry is past the end, and one float4
lost from one list's contribution to a shared id moves the applied weight by ten tolerances at least."""
from collections import Counter

import numpy as np
import pytest

import exchange_shape_cases as xc
import row_shape_cases as rc

TABLE_IDS = ["d%d_stride%d" % t for t in xc.TABLES]
F32, F64 = np.float32, np.float64


def in_levels(a):
    return bool(np.isin(np.abs(a) * 8, (1, 2, 3)).all())


def test_the_cases_reach_every_row_shape_twice():
    assert xc.WIDTHS == (4, 64, 68, 128, 132, 256, 260, 384, 388, 512, 516, 768, 772, 1024)
    assert xc.TABLES == tuple((d, d) for d in xc.WIDTHS) + ((257, 260),)
    for d4 in range(1, 257):
        assert xc.pick_row_shape(d4) == rc.pick_row_shape(d4)
    for shape, (first, last) in rc.ROW_SHAPES.items():
        assert xc.pick_row_shape(first // 4) == xc.pick_row_shape(last // 4) == shape
        assert first == 4 or xc.pick_row_shape(first // 4 - 1) != shape
        assert xc.pick_row_shape(last // 4 + 1) != shape
    assert Counter(xc.pick_row_shape(d // 4) for d in xc.WIDTHS) == {shape: 2 for shape in rc.ROW_SHAPES}
    assert xc.pick_row_shape(257 // 4) == (64, 1) and xc.pick_row_shape(260 // 4) == (32, 3)     # the padding crosses a boundary
    # the long lists: every lanes-per-row count, NV = 1 and NV > 1
    assert {xc.pick_row_shape(d // 4) for d in xc.LONG_WIDTHS.values()} == set(xc.LONG_WIDTHS) \
        == {(16, 1), (32, 1), (32, 3), (64, 1), (64, 4)}
    assert all(xc.pick_row_shape(d // 4)[0] in (16, 64) for d in xc.LONG_ADAM)
    assert {xc.pick_row_shape(d // 4)[0] for d in xc.LONG_ADAM} == {16, 64}


@pytest.mark.parametrize("n_lists", [6, 11])
@pytest.mark.parametrize("sides", [1, 2, 3])
@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_lists_hold_every_kind_and_every_id_set(dm, stride, sides, n_lists):
    c = xc.case(dm, stride, sides, n_lists)
    kinds = [l["kind"] for l in c.lists]
    assert len(kinds) == n_lists and kinds[:6] == ["bare", "bare", "bare", "header", "override", "empty"]
    assert Counter(kinds)["bare"] >= 3 and n_lists == 6 or (n_lists == 11 and "header" in kinds[8:])    # a header in the second launch
    G, Gb, count, first = xc.dense_reference(c)
    for s, bit in ((0, 1), (1, 2)):
        if not sides & bit:
            assert not count[s].any()
            continue
        # the three id sets, and a first namer that is not list 0 among the ids several lists name
        assert (count[s] == 0).sum() == xc.N_NONE and (count[s] >= 2).sum() == xc.N_SHARED and (count[s] == 1).sum() == 101
        assert count[s].max() <= 4 and (first[s][count[s] >= 2] > 0).any() and (first[s][count[s] >= 2] == 0).any()
    for k, l in enumerate(c.lists):
        e, ids, sds, n = l["entries"], l["ids"], l["sides"], len(l["ids"])
        assert e.shape == (n, stride + 4) and e.dtype == F32
        assert (n == 0) == (l["kind"] == "empty")
        if n == 0:
            continue
        assert in_levels(e[:, :dm]) and in_levels(e[:, stride]) and not e[:, dm:stride].any() and not e[:, stride + 3].any()
        assert (np.diff(sds.astype(int)) >= 0).all()                         # the row entries before the col entries
        assert ids.min() >= 0 and ids.max() < c.V
        for s in (0, 1):
            assert len(set(ids[sds == s].tolist())) == (sds == s).sum()      # distinct within a list and side
        stored_id, stored_side = e.view(np.int32)[:, stride + 1], e.view(np.int32)[:, stride + 2]
        if l["kind"] == "override":
            assert len(set(sds.tolist())) == 1 and l["fixed_side"] == sds[0] == (1 if sides & 2 else 0)
            assert (stored_id != ids).all() and (stored_side != sds).all()
            assert stored_id.min() >= 0 and stored_id.max() < c.V and set(stored_side.tolist()) <= {0, 1}     # wrong, in range
        else:
            assert (stored_id == ids).all() and (stored_side == sds).all()
            if sides == 3:
                assert set(sds.tolist()) == {0, 1}                           # rows and cols both occur
        if l["kind"] == "header":
            assert c.capacity > n and xc.header_of(l, stride).view(np.int32)[0, :2].sum() == n
            assert ((l["partials"] * 8) % 1 == 0).all()
    assert sum(len(l["ids"]) for l in c.lists) > 16 * 8                      # several workgroups at every shape


@pytest.mark.parametrize("n_lists", [6, 11])
@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_every_list_sum_is_exact_in_float32_in_either_order(dm, stride, n_lists):
    c = xc.case(dm, stride, 3, n_lists)
    G, Gb, count, first = xc.dense_reference(c)
    assert ((G * 8) % 1 == 0).all() and np.abs(G).max() <= 4 * 3 / 8 and not G[:, :, dm:].any()
    for order in (c.lists, c.lists[::-1]):
        acc, accb = np.zeros((2, c.V, stride), F32), np.zeros((2, c.V), F32)
        for l in order:
            for s in (0, 1):
                sel = l["sides"] == s
                acc[s][l["ids"][sel]] += l["entries"][sel, :stride]
                accb[s][l["ids"][sel]] += l["entries"][sel, stride]
        assert acc.dtype == F32 and (acc.astype(F64) == G).all() and (accb.astype(F64) == Gb).all()
    # the mark words: the count and 1 + the first namer; behind the count an id that one list names keeps the bare count
    words = xc.mark_words(count, first, True)
    assert ((words & 255) == count).all() and ((words >> 8)[count >= 2] == first[count >= 2] + 1).all()
    assert (words[count == 1] == 1).all() and (words[count == 0] == 0).all()
    bare = xc.mark_words(count, first, False)
    assert ((bare & 255) == 0).all() and ((bare >> 8) == first + 1).all()


@pytest.mark.parametrize("stride", sorted(xc.LONG_WIDTHS.values()))
def test_long_lists_give_groups_of_one_to_four_entries_and_a_pair_past_the_end(stride):
    lpr = xc.pick_row_shape(stride // 4)[0]
    T = xc.kMaxBlocks * (xc.kBlock // lpr)
    assert T == xc.lane_groups(stride) == {16: 32768, 32: 16384, 64: 8192}[lpr]
    counts = xc.long_counts(stride)
    assert counts == (3 * T + 2, 2 * T + 1, 2 * T, T)
    per_group = [xc.entries_per_group(n, T) for n in counts]
    assert all(p.sum() == n for p, n in zip(per_group, counts))
    assert set(np.concatenate(per_group).tolist()) == {1, 2, 3, 4}
    assert max(p.max() for p in per_group) <= lpr                            # one look-up round of the group's lanes
    # apply_packed_kernel moves two entries at a time: a group of an odd count has a pair whose second entry is past the end
    assert any((p % 2 == 1).any() for p in per_group) and (per_group[0] == 3).any() and (per_group[3] == 1).all()
    assert (per_group[1] == 3).sum() == 1 and (per_group[0] == 4).sum() == 2  # ... in one group only, and in all but two
    # the sweep of the dense-decay optimizers strides too: more rows than kSweepRows per lane group of a full grid
    V_side = 2 * T + 41
    assert 2 * V_side > xc.kSweepRows * T and V_side >= (counts[0] + 1) // 2
    if lpr == 16:
        assert 2 * V_side > 65536


@pytest.mark.parametrize("stride", [64, 132])
def test_long_case_names_ids_once_twice_and_never(stride):
    c = xc.long_case(stride)
    assert [len(l["ids"]) for l in c.lists] == list(xc.long_counts(stride)) and c.V == 2 * xc.lane_groups(stride) + 41
    G, Gb, count, first = xc.dense_reference(c)
    for s in (0, 1):
        share = np.bincount(count[s], minlength=5) / c.V
        assert share[0] > 0.03 and share[1] > 0.2 and share[2:].sum() > 0.4 and (first[s][count[s] >= 2] > 0).mean() > 0.1
    assert in_levels(c.lists[0]["entries"][:, :stride]) and ((G * 8) % 1 == 0).all() and np.abs(G).max() <= 1.5


@pytest.mark.parametrize("dm,stride", xc.TABLES, ids=TABLE_IDS)
def test_what_one_lost_float4_does_to_the_applied_weight(dm, stride):
    """On the float64 reference alone: the last float4 of a row (and, separately, the first) left out of one list's contribution
    to one shared id.  Under Adagrad the applied WEIGHT moves by 10 tolerances (atol + rtol |w| of the GPU test) at least,
    whichever id and list; under the other three optimizers the weight or a slot does (Adam and Adamax divide the gradient's
    size out of the weight's step: there it is m and v that show the loss)."""
    d4 = stride // 4
    for n_lists in (6, 11):
        c = xc.case(dm, stride, 3, n_lists)
        for opt in xc.OPTIMIZERS:
            low_w, low_any = (min(xc.removal_factors(c, opt, k4)[i].min() for k4 in (0, d4 - 1)) for i in (0, 1))
            print("d_model %d stride %d, %d lists, %s: one float4 lost moves the weight by %.1f tolerances at least, the weight "
                  "or a slot by %.1f" % (dm, stride, n_lists, opt, low_w, low_any))
            assert low_any >= 10
            if opt == "Adagrad":
                assert low_w >= 10
