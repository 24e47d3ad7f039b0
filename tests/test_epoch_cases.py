"""CPU side of tests/test_gpu_epoch_edges.py: the oracle functions the GPU tests compare against have the properties that
define them (oracle/glove_ref.py feistel_walk, build_masters, deal_epoch), and every case of tests/epoch_cases.py reaches
the branch its label names — by the restatement of the host decisions that sits next to the table."""
import numpy as np
import pytest

import epoch_cases as ec
import glove_ref as ref
from epoch_cases import KEY, KEYS, T


# ---- the oracle's own properties -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 65535, 65536, 65537, 2 ** 21])
def test_feistel_walk_is_a_permutation(n):
    for key in KEYS:
        seats = ref.feistel_walk(np.arange(n), n, key)
        assert seats.min() >= 0 and seats.max() < n
        assert (np.bincount(seats, minlength=n) == 1).all(), (n, hex(key))


def _key_tuples(major, minor):
    return list(zip(major.tolist(), minor.tolist()))


@pytest.mark.parametrize("case", [c for c in ec.MASTERS_CASES if c.n <= 5000], ids=lambda c: c.label)
def test_build_masters_gives_the_two_sorted_orders_and_their_link(case):
    row, col, _, _ = ec.masters_stream(case.n, case.V, case.V_row, case.ids)
    m = ref.build_masters(row, col, case.V, case.V_row or None)
    n = case.n
    Vr = case.V_row or case.V
    # ids outside their table count as id 0, everything else is kept
    r64, c64 = row.astype(np.int64), col.astype(np.int64)
    np.testing.assert_array_equal(m["row"], np.where((r64 < 0) | (r64 >= Vr), 0, r64))
    np.testing.assert_array_equal(m["col"], np.where((c64 < 0) | (c64 >= case.V), 0, c64))
    for perm, major, minor in ((m["perm_r"], m["row"], m["col"]), (m["perm_c"], m["col"], m["row"])):
        assert sorted(perm.tolist()) == list(range(n))
        keys = list(zip(major[perm].tolist(), minor[perm].tolist(), perm.tolist()))
        assert keys == sorted(keys)                         # sorted by (major, minor, stream index)
    np.testing.assert_array_equal(m["perm_r"][m["link"]], m["perm_c"])          # the same stream index at both positions
    assert sorted(m["link"].tolist()) == list(range(n))


@pytest.mark.parametrize("n,V,B", [(1, 5, 1), (100, 7, 1024), (2049, 50, 8), (5000, 300, 777), (5000, 300, 1), (6145, 40, 3)])
def test_deal_epoch_partitions_both_orders_by_the_same_batches(n, V, B):
    row, col, _, _ = ec.masters_stream(n, V)
    m = ref.build_masters(row, col, V)
    seen = []
    for key in KEYS:
        ir, ic = ref.deal_epoch(m, B, key)
        assert sorted(ir.tolist()) == list(range(n)) and sorted(ic.tolist()) == list(range(n))
        for lo in range(0, n, B):
            br, bc = ir[lo:lo + B], ic[lo:lo + B]
            assert sorted(br.tolist()) == sorted(bc.tolist())                   # the same pairs on both sides
            kr = list(zip(m["row"][br].tolist(), m["col"][br].tolist(), br.tolist()))
            kc = list(zip(m["col"][bc].tolist(), m["row"][bc].tolist(), bc.tolist()))
            assert kr == sorted(kr) and kc == sorted(kc)                        # (id, partner, stream index) on its own side
        seen.append(ir)
    if n > B and n >= 100:
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])      # two keys, two epochs


# ---- every case reaches the branch its label names -----------------------------------------------------------------------
def test_labels_are_unique():
    for table in (ec.MASTERS_CASES, ec.DEAL_CASES, ec.hand_cases(8), ec.SORTED_CASES):
        labels = [c.label for c in table]
        assert len(set(labels)) == len(labels)


@pytest.mark.parametrize("case", ec.MASTERS_CASES, ids=lambda c: c.label)
def test_masters_case_reaches_its_branch(case):
    row, col, w, _ = ec.masters_stream(case.n, case.V, case.V_row, case.ids)
    m = ref.build_masters(row, col, case.V, case.V_row or None)
    got = dict(ec.masters_decisions(case.V, case.V_row), tiles=max(-(-case.n // T), 1), partial_wave=case.n % 64 != 0,
               all_equal=len(set(_key_tuples(m["row"], m["col"]))) == 1, one_row=len(np.unique(m["row"])) == 1 and len(np.unique(m["col"])) > 1,
               distinct_pairs=len(set(_key_tuples(m["row"], m["col"]))))
    if case.ids == "planted":
        got["planted"] = all(v in row and v in col for v in ec.PLANTED(case.V, case.V_row))
        assert ec.mapped_count(row, col, case.V, case.V_row) >= 2 * 12 * 4         # (V_row itself is a valid col id)
    for k, v in case.expect.items():
        assert got[k] == v, (case.label, k, got[k], v)
    assert len(np.unique(w)) == case.n                      # all w distinct: equal keys in the wrong order show
    if case.ids == "uniform" and case.n >= 2:
        # ids over the whole table: the top bit of every field is set somewhere, so the last pass of a field does sort
        assert m["col"].max() == case.V - 1 and m["row"].max() == (case.V_row or case.V) - 1
    if case.ids == "uniform" and case.n >= 5000 and case.V >= 2048:
        assert len(np.unique(m["col"] >> (ec.ceil_log2(case.V) - 3))) >= 5      # (and the high digits are populated, not one value)
    if got["all_equal"]:
        np.testing.assert_array_equal(m["perm_r"], np.arange(case.n))           # ties: the stream order, link the identity
        np.testing.assert_array_equal(m["link"], np.arange(case.n))
    if case.label == "one_digit_takes_every_tile":
        assert case.n >= 3 * T          # every lane of every wave of a whole tile is a peer of the row-major order's major passes


def test_masters_pass_counts_switch_where_the_table_says():
    assert [ec.masters_decisions(V)["P"] for V in (1, 2048, 2049, 1 << 22, (1 << 22) + 1, ec.INT32_MAX)] == [1, 1, 2, 2, 3, 3]
    assert not ec.masters_decisions(5000, 5000)["empty_pass"] and ec.masters_decisions(5000, 2)["empty_pass"]


@pytest.mark.parametrize("case", ec.DEAL_CASES, ids=lambda c: c.label)
def test_deal_case_reaches_its_branch(case):
    got = ec.deal_decisions(case.n, case.B)
    assert not got["refused"]
    for k, v in case.expect.items():
        assert got[k] == v, (case.label, k, got[k], v)
    assert set(case.keys) <= set(KEYS) and KEY in case.keys


def test_deal_cases_cover_every_switch():
    d = [ec.deal_decisions(c.n, c.B) for c in ec.DEAL_CASES]
    nbs = {x["nb"] for x in d}
    assert {256, 257, 2048, 2049} <= nbs                    # cache8 and the pass count, both sides of each switch
    assert {(x["passes"], x["bshift"] >= 0) for x in d} == {(1, True), (1, False), (2, True), (2, False)}
    assert {x["nt"] for x in d} == {True, False} and max(x["tiles"] for x in d) > 2048
    assert {(x["nt"], x["bshift"] >= 0) for x in d} >= {(True, True), (True, False)}
    assert any(c.B > c.n for c in ec.DEAL_CASES) and any(c.B == 1 for c in ec.DEAL_CASES)
    assert {c.n - c.B for c in ec.DEAL_CASES} >= {-1, 0, 1}
    assert {c.n for c in ec.DEAL_CASES} >= {1, T - 1, T, T + 1}
    assert ec.deal_decisions(*ec.REFUSED_DEAL)["refused"] and not ec.deal_decisions(1 << 22, 1)["refused"]


@pytest.mark.parametrize("case", ec.hand_cases(8), ids=lambda c: c.label)
def test_hand_made_batches_have_the_listed_runs(case):
    rs, cs = ec.hand_epoch(case.row_runs, case.col_runs)
    B = sum(case.row_runs)
    assert len(rs[0]) == ec.HAND_BATCHES * B
    for b in range(ec.HAND_BATCHES):
        sl = slice(b * B, (b + 1) * B)
        assert ec.run_lengths(rs[0][sl]) == case.row_runs and ec.run_lengths(cs[0][sl]) == case.col_runs
        # both sides hold the same pairs; the col side is the stable sort of the row side by col id
        order = np.argsort(rs[1][sl], kind="stable")
        for f_r, f_c in ((1, 0), (0, 1), (2, 2), (3, 3)):
            np.testing.assert_array_equal(rs[f_r][sl][order], cs[f_c][sl])
    assert max(rs[0].max(), cs[0].max()) < ec.hand_vocab(case)
    if len(case.col_runs) > 1 and B > 8:
        assert not np.array_equal(rs[1][:B], rs[1][B:2 * B])                    # another shuffle per batch


def test_hand_made_batches_cover_every_edge():
    from trainer.hip_api import HEAVY_CHUNKS as H
    cases = {c.label: c for c in ec.hand_cases(H)}
    starts = lambda runs: np.r_[0, np.cumsum(runs)]          # noqa: E731
    c = cases["runs_64_65_63_at_tile_edges"]
    s = starts(c.row_runs).tolist()
    runs = dict(zip(s, c.row_runs))
    assert runs[T - 64] == 64 and runs[T] == 65             # a run of 64 ends on a tile edge, one of 65 starts on it
    assert s[5] % T != 0 and runs[s[5]] == T                # a whole tile's worth of one id across an edge
    assert runs[s[6]] == 3 * T + 1 and (s[6] + runs[s[6]]) // T - s[6] // T >= 3          # over several tiles: the search loop
    c = cases["runs_65_63_end_on_tile_edges"]
    s = starts(c.row_runs).tolist()
    assert s[2] == T and s[4] == 2 * T and c.row_runs[1] == 65 and c.row_runs[3] == 63 and s[5] % T == 3
    for cap in ec.CAP_EDGE_CAPS:
        c = cases["cap_%d_heavy_edge" % cap]
        row = np.repeat(np.arange(len(c.row_runs)), c.row_runs)
        plan = ref.build_plan(row, row, cap, heavy_chunks=H)
        chunks = plan["r_uniq_rec"][:, 2].tolist()
        assert H in chunks and H + 1 in chunks and plan["counts"][4] == 2      # exactly H chunks is not heavy, one pair more is
        assert {cap, cap + 1} <= set(c.row_runs)
    sizes = {sum(c.row_runs) for c in cases.values()}
    assert {1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1} <= sizes
    assert any(len(c.row_runs) == sum(c.row_runs) == T + 1 for c in cases.values())         # all ids distinct
    assert any(B % 2 for B in sizes) and any(B % 4 == 2 for B in sizes)       # batch starts off 16-byte alignment
    assert {(f * 1) % 4 for f, _ in ec.HAND_RUNS} == {0, 1, 2}


def test_sorted_and_step_cases_cover_small_and_odd_batches():
    Bs = {c.B for c in ec.SORTED_CASES}
    assert {1, 7, 63, 65, 2047, 2049, 4097} <= Bs
    for c in ec.SORTED_CASES:
        assert c.n // c.B >= 3
    assert set(ec.STEP_BATCH_SIZES) <= Bs and set(ec.STEP_FORMS) == set(ec.PLAN_KINDS)


def test_fuzz_cases_stay_inside_their_table():
    kinds, seen_B = set(), set()
    for seed in range(24):
        c = ec.fuzz_case(seed)
        assert c["n"] in ec.FUZZ_N and c["V"] in ec.FUZZ_V and 0 <= c["V_row"] < max(c["V"], 1) and 1 <= c["cap"] <= 32
        assert c["count"] <= ec.FUZZ_MAX_PLANS and (c["first"] + c["count"]) * c["B"] <= c["n"]
        assert not ec.deal_decisions(c["n"], c["B"])["refused"]
        assert ec.fuzz_case(seed) == c
        kinds.add(c["kind"])
        seen_B.add(c["B"])
    assert kinds == set(ec.PLAN_KINDS) and len(seen_B) >= 4
