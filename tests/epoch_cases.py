"""TEST-ONLY case table of tests/test_gpu_epoch_edges.py: the shapes at which the dealt-epoch kernels (glove_masters_build,
glove_epoch_deal, glove_plan_build_sorted) take another branch, seeded generators of their inputs, and a Python restatement
of the host decisions every case relies on (deal_plan, glove_epoch_deal and glove_masters_build of csrc/glove_epoch.hip).
tests/test_epoch_cases.py proves on the CPU that every case reaches the branch its label names, and pins the oracle functions
(oracle/glove_ref.py feistel_walk / build_masters / deal_epoch) the GPU tests compare against.  Never imported by the product.

All of it is integer work: the GPU tests compare bit for bit, so w is a permutation of 1 .. n as float32 (all distinct: a
pair that lands in the wrong place, or two equal keys in the wrong order, shows in w) and y is any float32."""
import functools
from typing import NamedTuple

import numpy as np

import glove_ref as ref
from helpers import zipf_ids

T = 2048                            # positions of a counting-sort tile (kCsThreads x 8) and of a numbering tile (kTile)
MAX_BITS = 11                       # kCsMaxBits: 2,048 digits a pass
KEY = 0x0123456789abcdef_fedcba9876543210
KEYS = (0, KEY, 2 ** 128 - 1)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NT_BYTES = 128 << 20                # both orders in and out, 64 B per pair: from here on the deal's loads and stores are non-temporal


# ---- the host decisions, restated ------------------------------------------------------------------------------------
def ceil_log2(v):
    """ceil_log2_64 of csrc/glove_epoch.hip: b >= 1 with 2^b >= v."""
    b = 1
    while (1 << b) < v:
        b += 1
    return b


def deal_decisions(n, B):
    """What deal_plan and glove_epoch_deal decide on the host for n pairs in batches of B."""
    nb = -(-n // B)
    bits = ceil_log2(max(nb, 2))
    passes = 1 if bits <= MAX_BITS else 2
    db = (bits, 0) if passes == 1 else ((bits + 1) // 2, bits - (bits + 1) // 2)
    return dict(nb=nb, bits=bits, passes=passes, db=db, refused=max(db) > MAX_BITS, cache8=nb <= 256,
                bshift=B.bit_length() - 1 if B & (B - 1) == 0 else -1, nt=n * 64 >= NT_BYTES, tiles=max(-(-n // T), 1),
                partial_wave=n % 64 != 0, full_batches=n // B)


def masters_decisions(V, V_row=0):
    """What glove_masters_build decides on the host: passes per field P (the same for both orders and both fields) and
    whether some pass of some order covers no bits (digit 0 for everybody, db = 1, mask = 0)."""
    Vr = V_row or V
    bits = ((ceil_log2(V), ceil_log2(Vr)), (ceil_log2(Vr), ceil_log2(V)))          # [order][0 minor, 1 major]
    P = -(-max(max(b) for b in bits) // MAX_BITS)
    empty = False
    for order in bits:
        for fb in order:
            per = -(-fb // P)
            for q in range(P):
                lo = min(q * per, fb)
                empty |= min(lo + per, fb) - lo == 0
    return dict(P=P, empty_pass=empty, bits=bits)


def payload(rng, n):
    return (rng.permutation(n) + 1).astype(np.float32), rng.standard_normal(n).astype(np.float32)


# ---- glove_masters_build -----------------------------------------------------------------------------------------------
class MastersCase(NamedTuple):
    label: str
    n: int
    V: int
    V_row: int
    ids: str                        # "uniform" over the whole table | "one_row" | "three_pairs" | "planted"
    expect: dict                    # entries of masters_decisions(V, V_row) / of the tile geometry the label names


MASTERS_CASES = (
    MastersCase("n1", 1, 5, 0, "uniform", dict(tiles=1)),
    MastersCase("n2_one_id", 2, 1, 0, "uniform", dict(tiles=1, all_equal=True)),
    MastersCase("tile_minus_1_partial_wave", T - 1, 50, 0, "uniform", dict(tiles=1, partial_wave=True)),
    MastersCase("tile_exact", T, 50, 0, "uniform", dict(tiles=1, partial_wave=False)),
    MastersCase("tile_plus_1", T + 1, 50, 0, "uniform", dict(tiles=2, partial_wave=True)),
    MastersCase("four_tiles", 3 * T + 5, 50, 0, "uniform", dict(tiles=4)),
    MastersCase("one_pass_per_field_last", 5000, 2048, 0, "uniform", dict(P=1, empty_pass=False)),
    MastersCase("two_passes_per_field_first", 5000, 2049, 0, "uniform", dict(P=2, empty_pass=False)),
    MastersCase("two_passes_per_field_last", 5000, 4194304, 0, "uniform", dict(P=2, empty_pass=False)),
    MastersCase("three_passes_per_field_first", 5000, 4194305, 0, "uniform", dict(P=3, empty_pass=False)),
    MastersCase("pass_without_bits_vrow2", 5000, 5000, 2, "uniform", dict(P=2, empty_pass=True)),
    MastersCase("pass_without_bits_vrow1", 5000, 3000, 1, "uniform", dict(P=2, empty_pass=True)),
    MastersCase("vrow_equals_v", 5000, 3000, 3000, "uniform", dict(P=2, empty_pass=False)),
    MastersCase("one_digit_takes_every_tile", 3 * T + 5, 300, 0, "one_row", dict(tiles=4, one_row=True)),
    MastersCase("all_keys_equal_ties_by_stream_index", 3 * T + 5, 1, 0, "uniform", dict(tiles=4, all_equal=True)),
    MastersCase("three_pairs_stable_in_w", 5000, 7, 0, "three_pairs", dict(distinct_pairs=3)),
    MastersCase("ids_int32_min_max_v_vrow", 5000, 300, 120, "planted", dict(planted=True)),
)

PLANTED = lambda V, V_row: (INT32_MIN, -1, INT32_MAX, V, V_row)          # noqa: E731  (in row and in col)


@functools.lru_cache(maxsize=None)
def masters_stream(n, V, V_row=0, ids="uniform", seed=0):
    """(row, col, w, y) of a case, read-only."""
    rng = np.random.default_rng(1000003 * seed + 7919 * n + V + 31 * V_row + len(ids))
    Vr = V_row or V
    row, col = rng.integers(0, Vr, n).astype(np.int32), rng.integers(0, V, n).astype(np.int32)
    if n >= 2:
        row[n // 2], col[n // 3] = Vr - 1, V - 1            # the last id of either table: the top bit of every field is in use
    if ids == "one_row":
        row[:] = Vr - 1                                     # (the high digit bits set as well)
    elif ids == "three_pairs":
        pairs = np.array([(5, 2), (2, 5), (5, 6)], np.int32)
        pick = rng.integers(0, 3, n)
        row, col = pairs[pick, 0].copy(), pairs[pick, 1].copy()
    elif ids == "planted":
        vals = np.array(PLANTED(V, V_row), np.int64).astype(np.int32)
        row[rng.choice(n, 60, replace=False)] = np.tile(vals, 12)
        col[rng.choice(n, 60, replace=False)] = np.tile(vals, 12)
    elif ids == "zipf":
        row, col = zipf_ids(rng, n, Vr), zipf_ids(rng, n, V)
    elif ids != "uniform":
        raise ValueError(ids)
    w, y = payload(rng, n)
    for a in (row, col, w, y):
        a.setflags(write=False)
    return row, col, w, y


def mapped_count(row, col, V, V_row=0):
    """Ids outside their table (they count as id 0): what glove_masters_build reports."""
    row, col = row.astype(np.int64), col.astype(np.int64)
    return int(((row < 0) | (row >= (V_row or V))).sum() + ((col < 0) | (col >= V)).sum())


# ---- glove_epoch_deal ------------------------------------------------------------------------------------------------
class DealCase(NamedTuple):
    label: str
    n: int
    B: int
    V: int
    keys: tuple
    expect: dict                    # entries of deal_decisions(n, B)


def _deal(label, n, B, V=300, keys=KEYS, **expect):
    return DealCase(label, n, B, V, keys, expect)


DEAL_CASES = (
    _deal("n1_B1", 1, 1, nb=1, passes=1, bshift=0),
    _deal("n1_B4_B_beyond_n", 1, 4, nb=1, full_batches=0, bshift=2),
    _deal("n2_B1", 2, 1, nb=2, bits=1),
    _deal("B_beyond_n", 100, 1024, nb=1, full_batches=0, partial_wave=True),
    _deal("tile_minus_1_cache8", T - 1, 8, tiles=1, nb=256, cache8=True, bshift=3, passes=1),
    _deal("tile_exact_cache8_last", T, 8, tiles=1, nb=256, cache8=True, bshift=3, passes=1, partial_wave=False),
    _deal("tile_plus_1_cache32_first", T + 1, 8, tiles=2, nb=257, cache8=False, bshift=3, passes=1),
    _deal("four_tiles_B_tile", 3 * T + 5, 2048, tiles=4, nb=4, bshift=11),
    _deal("one_pass_last_division", 6144, 3, nb=2048, passes=1, bshift=-1, cache8=False),
    _deal("two_passes_first_division", 6145, 3, nb=2049, passes=2, bshift=-1, db=(6, 6)),
    _deal("two_passes_first_bshift", 8196, 4, nb=2049, passes=2, bshift=2),
    _deal("B1_two_passes_bshift", 5000, 1, nb=5000, passes=2, bshift=0, db=(7, 6)),
    _deal("odd_B_one_pass_division", 5000, 777, nb=7, passes=1, bshift=-1, cache8=True),
    _deal("one_pass_bshift", 5000, 1024, nb=5, passes=1, bshift=10),
    _deal("B_n_minus_1", 5000, 4999, nb=2, full_batches=1),
    _deal("B_equals_n", 5000, 5000, nb=1, full_batches=1),
    _deal("B_n_plus_1", 5000, 5001, nb=1, full_batches=0),
    _deal("nt_last_without", 2 ** 21 - 1, 2 ** 17, V=50000, keys=(KEY,), nt=False, tiles=1024, bshift=17, cache8=True),
    _deal("nt_first_division", 2 ** 21, 2 ** 17 + 1, V=50000, keys=(KEY,), nt=True, tiles=1024, bshift=-1),
    _deal("nt_scan_carry_beyond_2048_tiles", 2 ** 22 + 2049, 2 ** 18, V=100000, keys=(KEY,), nt=True, tiles=2050, bshift=18),
)
REFUSED_DEAL = (2 ** 22 + 1, 1)     # more than 2^22 batches: a digit of 12 bits


# ---- glove_plan_build_sorted: hand-made batches ------------------------------------------------------------------------
class HandCase(NamedTuple):
    label: str
    row_runs: tuple                 # run lengths of the row side, in id order
    col_runs: tuple                 # run lengths of the col side, in id order (after the stable sort)
    caps: tuple                     # chunk caps to build it with


def _hand(label, runs, caps=(7,), col_runs=None):
    return HandCase(label, tuple(runs), tuple(runs if col_runs is None else col_runs), tuple(caps))


def cap_edge_runs(cap, H):
    """Runs at the chunk cap's and the heavy threshold's edges: H chunks exactly (not heavy) against one pair more (heavy)."""
    return tuple(x for x in (cap, cap + 1, cap - 1, H * cap, H * cap + 1, 1) if x > 0)


CAP_EDGE_CAPS = (1, 2, 7, 8, 9, 32)


def hand_cases(H):
    """`H`: the plan's heavy_chunks (ids of more chunks are reduced by a whole workgroup)."""
    return (
        _hand("B1_one_pair", [1]),
        _hand("B2_one_id", [2]),
        _hand("B2_distinct", [1, 1]),
        _hand("run_63_is_the_batch", [63]),
        _hand("run_64_is_the_batch", [64]),
        _hand("run_65_is_the_batch", [65]),
        _hand("one_id_tile_minus_1", [T - 1]),
        _hand("one_id_one_tile", [T]),
        _hand("one_id_tile_plus_1", [T + 1]),
        _hand("one_id_over_four_tiles_search_loop", [3 * T + 1]),
        _hand("all_distinct_B2049", [1] * (T + 1)),
        _hand("all_distinct_rows_one_col_id", [1] * (T + 1), col_runs=[T + 1]),
        _hand("one_row_id_all_distinct_cols", [T + 1], col_runs=[1] * (T + 1)),
        _hand("runs_64_65_63_at_tile_edges", [T - 64, 64, 65, 63, 1, T, 3 * T + 1, 1, 1, 130], caps=(7, 1, 32)),
        _hand("runs_65_63_end_on_tile_edges", [T - 65, 65, T - 63, 63, 5 * T + 3, 1], caps=(7, 1, 32)),
        _hand("long_run_between_single_pairs", [1, 5 * T + 3, 1], caps=(7, 1, 32)),
    ) + tuple(_hand("cap_%d_heavy_edge" % cap, cap_edge_runs(cap, H), caps=(cap,)) for cap in CAP_EDGE_CAPS)


HAND_BATCHES = 3
HAND_RUNS = ((0, 3), (1, 2), (2, 1))        # (first batch, batches): batch starts and first_pair take every residue
PLAN_KINDS = ("records", "words", "borrow")


def plan_kind_args(kind):
    """Keyword arguments of GloveHip.staging_plan for a plan kind."""
    return dict(records=dict(records=True), words=dict(records=False, run_words=True),
                borrow=dict(records=False, run_words=True, borrow=True))[kind]


@functools.lru_cache(maxsize=None)
def hand_epoch(row_runs, col_runs, nb=HAND_BATCHES, seed=0):
    """nb consecutive batches with these run lengths (another shuffle of the col ids each) as the two orders of a dealt epoch
    would hold them: (row_side, col_side), each (id, partner, w, y) of nb B entries.  The row side is the arrival order; the
    col side is its stable sort by col id (oracle build_plan's c_perm)."""
    B = sum(row_runs)
    assert sum(col_runs) == B
    rng = np.random.default_rng(77 + 13 * seed + B + len(row_runs))
    sides = [[], []]
    for _ in range(nb):
        row = np.repeat(np.arange(len(row_runs)), row_runs).astype(np.int32)
        col = rng.permutation(np.repeat(np.arange(len(col_runs)), col_runs)).astype(np.int32)
        w, y = payload(rng, B)
        plan = ref.build_plan(row, col, B)
        assert (plan["perm_r"] == np.arange(B)).all()
        cp = plan["c_perm"]
        sides[0].append((row, col, w, y))
        sides[1].append((col[cp], row[cp], w[cp], y[cp]))
    out = tuple(tuple(np.concatenate([b[f] for b in side]) for f in range(4)) for side in sides)
    for side in out:
        for a in side:
            a.setflags(write=False)
    return out


def hand_vocab(case):
    return max(len(case.row_runs), len(case.col_runs)) + 2


def run_lengths(sorted_ids):
    """Lengths of the runs of equal ids."""
    ids = np.asarray(sorted_ids)
    edges = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1], True])
    return tuple(int(x) for x in np.diff(edges))


# ---- glove_plan_build_sorted behind the deal -------------------------------------------------------------------------------
class SortedCase(NamedTuple):
    label: str
    n: int
    V: int
    B: int
    cap: int


SORTED_CASES = tuple(SortedCase("B%d_%s" % (B, what), 5 * B + 3, 40, B, 4) for B, what in (
    (1, "one_pair"), (7, "below_a_wave_odd"), (63, "wave_minus_1"), (65, "wave_plus_1_odd"), (2047, "tile_minus_1"),
    (2049, "tile_plus_1_odd"), (4097, "two_tiles_plus_1_odd"))) + (
    SortedCase("one_id_three_tiles_every_batch", 3 * 4097 + 1, 1, 4097, 7),
    SortedCase("nearly_all_distinct_cap1", 6000, 20000, 2000, 1),
)
STEP_BATCH_SIZES = (1, 63, 2049)
STEP_V, STEP_D, STEP_CAP = 40, 16, 4
STEP_FORMS = dict(records=(0,), words=(3, 4), borrow=(3, 4))     # (form 4 on twinned tables)


# ---- fuzz ------------------------------------------------------------------------------------------------------------------
FUZZ_N = (1, 2, 100, 2047, 2048, 2049, 6145, 20000)
FUZZ_V = (1, 3, 50, 2049, 300000)
FUZZ_B = (1, 3, 64, 777, 2048, 2049, "n")
FUZZ_MAX_PLANS = 4


def fuzz_case(seed):
    rng = np.random.default_rng(424242 + seed)
    n, V = int(rng.choice(FUZZ_N)), int(rng.choice(FUZZ_V))
    V_row = int(rng.integers(1, V)) if V > 1 and rng.integers(0, 2) else 0
    B = FUZZ_B[int(rng.integers(0, len(FUZZ_B)))]
    B = n if B == "n" else int(B)
    full = n // B
    first = int(rng.integers(0, full)) if full else 0
    return dict(seed=seed, n=n, V=V, V_row=V_row, B=B, cap=int(rng.integers(1, 33)), ids=("uniform", "zipf")[int(rng.integers(0, 2))],
                bad=bool(rng.integers(0, 2)), kind=PLAN_KINDS[int(rng.integers(0, 3))], first=first,
                count=min(FUZZ_MAX_PLANS, full - first) if full else 0, key=int(rng.integers(0, 2 ** 63)) << 64 | int(rng.integers(0, 2 ** 63)))


def fuzz_stream(c):
    """(row, col, w, y) of a fuzz case (fresh arrays)."""
    row, col, w, y = (a.copy() for a in masters_stream(c["n"], c["V"], c["V_row"], c["ids"], seed=c["seed"] + 1))
    if c["bad"]:
        row[::17] = c["V"] + 3
        col[5::29] = -2
        row[3::41] = INT32_MIN
    return row, col, w, y
