"""TEST-ONLY generator of the cases of tests/test_gpu_exchange_row_shapes.py: packed lists of several ranks for the kernels of
the touched-rows and dense exchange (csrc/glove_step.hip: count_packed_kernel, combine_packed_kernel, decay_unmarked_kernel,
apply_packed_kernel, gather_rows_kernel, dense_grad_kernel, pack_grad_kernel) at the first and the last width of each of the
seven row shapes of pick_row_shape and at 257 model columns on a stride of 260, and the float64 references on them.
tests/test_exchange_shape_cases.py proves on the references alone what the GPU tests rely on.  Never imported by the product.

Exact lists.  Every element of a gradient row and every bias gradient is one of {+-1, +-2, +-3} / 8 (no zero: a dropped
element always changes the sum), an id is named by at most four lists (at most eleven lists in all): every partial sum over
lists is a multiple of 1/8 below 2^2, exact in float32 in any order, so the dense buffer is compared for EQUALITY with float64.

The lists of a case (entry = [row, stride floats | bias gradient | id | side | 0], csrc/glove_step.hip "Touched-rows exchange"):
  bare      a run of entries that name their side (glove_packed_list.side = -1), the count on the host
  header    entry 0 is a header [row entries, col entries | four loss partials]; the count is read from it on the device and the
            launches are sized by capacity_entries, which lies above every count
  override  the ids come from glove_packed_list.ids and the side is fixed; the id and the side stored in the entries are
            WRONG on purpose (another id of the table, the other side: in range, so a kernel that read them would write a
            wrong row, not out of bounds)
  empty     no entries
Within a list the row entries come before the col entries (as pack_grad_kernel writes them), in random id order.  The ids of
each side split into three sets: named by exactly one list, named by two to four lists (the first of them is not always list
0), named by no list."""
import functools

import numpy as np

import glove_ref as ref
import row_shape_cases as rc

ROW_SHAPES, WIDTHS, TABLES, LEVELS = rc.ROW_SHAPES, rc.WIDTHS, rc.TABLES, rc.LEVELS
RTOL, ATOL = 1e-5, 1e-6             # helpers.assert_opt_tables_close's defaults: the tolerance of the apply on the GPU
V = 211                             # ids per side: a prime, some 120 entries per list — several workgroups at every shape
N_NONE, N_SHARED = 40, 70           # of the V ids of a side: named by no list, by two to four; the other 101 by exactly one
KINDS = ("bare", "bare", "bare", "header", "override", "empty")                 # the six lists of a case, in list (rank) order
KINDS_11 = KINDS + ("header", "bare", "bare", "header", "bare")                 # more than one launch of eight lists
OPTIMIZERS = ("Adagrad", "Adam", "RMSprop", "Adamax")
LR = {"Adagrad": 0.05, "Adam": 0.01, "RMSprop": 0.01, "Adamax": 0.01}
STEP = 3                            # global_step before the step under test
TAIL = (0.375, 2.0, 5.0, 1.0)       # the summed loss partials handed to the apply: sum e first
kBlock, kMaxBlocks, kSweepRows, kMarkCountBits = 256, 2048, 2, 8                # csrc/glove_common.h, csrc/glove_step.hip

# the long lists: one width for each lanes-per-row count and for NV = 1 and NV > 1
LONG_WIDTHS = {(16, 1): 64, (32, 1): 68, (32, 3): 260, (64, 1): 132, (64, 4): 772}
LONG_ADAM = (64, 132, 772)          # LPR 16 and LPR 64: Adam as well, so that decay_unmarked_kernel's strided sweep runs


def pick_row_shape(d4):
    """csrc/glove_common.h:pick_row_shape restated: the listed shape with the fewest slots that holds d4 float4."""
    best = None
    for lpr, nv in [(16, 1), (32, 1), (64, 1), (32, 3), (64, 2), (64, 3), (64, 4)]:
        if lpr * nv >= d4 and (best is None or lpr * nv < best[0] * best[1]):
            best = (lpr, nv)
    return best


def _levels(rng, *shape):
    return LEVELS[rng.integers(0, len(LEVELS), shape, dtype=np.uint8)]


def _entries(rng, dm, stride, ids, side):
    """[len(ids), stride + 4] float32: exact gradient rows (padding columns zero) and bias gradients of `ids` on `side`."""
    e = np.zeros((len(ids), stride + 4), np.float32)
    e[:, :dm] = _levels(rng, len(ids), dm)
    e[:, stride] = _levels(rng, len(ids))
    e.view(np.int32)[:, stride + 1] = ids
    e.view(np.int32)[:, stride + 2] = side
    return e


class PackedCase:
    """lists[k] = dict(kind, entries [n, stride + 4] float32, ids int32 [n] (the TRUE ids), sides int8 [n] (the TRUE sides),
    partials float32[4] (header lists), fixed_side); capacity: capacity_entries of the calls; V ids per side."""

    def __init__(self, dm, stride, lists, V_side, capacity):
        self.dm, self.stride, self.lists, self.V, self.capacity = dm, stride, lists, V_side, capacity


@functools.lru_cache(maxsize=None)
def case(dm, stride, sides=3, n_lists=6):
    """The lists of one width for an apply that covers `sides` (1 row side, 2 col side, 3 both): only those sides occur."""
    rng = np.random.default_rng(1000 * n_lists + 10 * dm + sides)
    kinds = KINDS if n_lists == 6 else KINDS_11
    assert len(kinds) == n_lists
    side_list = [s for s, bit in ((0, 1), (1, 2)) if sides & bit]
    fixed = side_list[-1]                                # the override list's side: the col side where it is covered
    holders = {s: [k for k, kind in enumerate(kinds) if kind != "empty" and (kind != "override" or s == fixed)] for s in side_list}
    named = {s: [[] for _ in kinds] for s in side_list}
    for s in side_list:
        perm = rng.permutation(V)
        for i in perm[N_NONE:N_NONE + N_SHARED]:
            for k in rng.choice(holders[s], int(rng.integers(2, 5)), replace=False):
                named[s][k].append(i)
        for i in perm[N_NONE + N_SHARED:]:
            named[s][int(rng.choice(holders[s]))].append(i)
    lists = []
    for k, kind in enumerate(kinds):
        parts, ids, sds = [], [], []
        for s in side_list:
            own = rng.permutation(np.array(named[s][k], np.int32))
            parts.append(_entries(rng, dm, stride, own, s))
            ids.append(own)
            sds.append(np.full(len(own), s, np.int8))
        e = np.concatenate(parts)
        ids, sds = np.concatenate(ids).astype(np.int32), np.concatenate(sds)
        if kind == "override":                           # what the entries store is wrong, in range
            e.view(np.int32)[:, stride + 1] = (ids + 1) % V
            e.view(np.int32)[:, stride + 2] = 1 - fixed
        partials = (rng.integers(-8, 9, 4) / 8).astype(np.float32) if kind == "header" else None
        for a in (e, ids, sds):
            a.setflags(write=False)
        lists.append(dict(kind=kind, entries=e, ids=ids, sides=sds, partials=partials, fixed_side=fixed if kind == "override" else -1))
    capacity = max(len(l["ids"]) for l in lists if l["kind"] == "header") + 5
    return PackedCase(dm, stride, tuple(lists), V, capacity)


def header_of(lst, stride):
    """[1, stride + 4] float32: the header entry of a list (row entries, col entries as int bits, the four loss partials)."""
    h = np.zeros((1, stride + 4), np.float32)
    h.view(np.int32)[0, 0] = int((lst["sides"] == 0).sum())
    h.view(np.int32)[0, 1] = int((lst["sides"] == 1).sum())
    if lst["partials"] is not None:
        h[0, 2:6] = lst["partials"]
    return h


def dense_reference(c):
    """What count + the combines in list order leave, in float64: G [2, V, stride] and Gb [2, V] (side 0 rows, 1 cols) the
    sums over the lists, count [2, V] how many lists name an id, first [2, V] the first of them (-1: none)."""
    G, Gb = np.zeros((2, c.V, c.stride)), np.zeros((2, c.V))
    count, first = np.zeros((2, c.V), np.int64), np.full((2, c.V), -1, np.int64)
    for k, l in enumerate(c.lists):
        for s in (0, 1):
            sel = l["sides"] == s
            ids = l["ids"][sel]                          # distinct within a list and side: fancy-index += is enough
            G[s][ids] += l["entries"][sel, :c.stride]
            Gb[s][ids] += l["entries"][sel, c.stride]
            count[s][ids] += 1
            fresh = ids[first[s][ids] < 0]
            first[s][fresh] = k
    return G, Gb, count, first


def mark_words(count, first, counted):
    """The mark of every id after the combines (csrc/glove_step.hip: bits 0..7 the count, bits 8.. 1 + the tag of the first list
    that stored the id's row): behind count_packed an id that ONE list names skips the dense buffer — combine leaves its
    mark at the bare count 1 and no tag; without count_packed the count bits stay zero and every named id carries its tag."""
    tag = np.where(first >= 0, (first + 1) << kMarkCountBits, 0)
    if not counted:
        return tag
    return np.where(count >= 2, count | tag, count)


def gradients_of(c, G, Gb, count, sum_e):
    """The `gr` of glove_ref.apply_update on the model's columns."""
    return dict(G_R=G[0][:, :c.dm].copy(), G_C=G[1][:, :c.dm].copy(), G_br=Gb[0].copy(), G_bc=Gb[1].copy(),
                touched_r=count[0] > 0, touched_c=count[1] > 0, sum_e=float(sum_e))


def seeded_tables(V_side, dm, optimizer, seed=11):
    """float64 oracle tables of float32 values at global_step STEP: weights in (-0.5, 0.5) and slots of the size of the squared
    gradients, so that a lost float4 moves the weight and not only the slot (tests/test_exchange_shape_cases.py)."""
    rng = np.random.default_rng(seed + dm)
    t = ref.Tables(V_side, dm, optimizer, dtype=np.float32, seed=seed)
    f = np.float32

    def uniform(lo, hi, shape):
        return (f(lo) + f(hi - lo) * rng.random(shape, dtype=f)).astype(f)
    for n in ("R", "C", "br", "bc"):
        shape = getattr(t, n).shape
        setattr(t, n, uniform(-0.5, 0.5, shape))
        if optimizer in ("Adam", "Adamax"):
            setattr(t, "M_" + n, uniform(-0.2, 0.2, shape))
            setattr(t, "V_" + n, uniform(0.05, 1.0, shape))
        else:
            setattr(t, "A_" + n, uniform(0.5, 2.0, shape))
    t.g = f(0.25)
    if optimizer in ("Adam", "Adamax"):
        t.M_g, t.V_g = f(0.125), f(0.5)
    else:
        t.A_g = f(0.75)
    t = t.astype(np.float64)
    t.step = STEP
    return t


def updated(optimizer, W, S1, S2, G, step=STEP):
    """The oracle's element update of one step on arrays of any shape (every element `touched`): (W, S1, S2) afterwards."""
    hp = ref.Hyper(learning_rate=LR[optimizer])
    dt = np.float64
    lr, eps = dt(np.float32(hp.learning_rate)), dt(np.float32(hp.epsilon))
    b1, b2 = dt(np.float32(hp.beta1)), dt(np.float32(hp.beta2))
    W, S1, S2 = W.copy(), S1.copy(), None if S2 is None else S2.copy()
    every = np.ones(W.shape[0], bool)
    tt = step + 1
    if optimizer == "Adagrad":
        ref._adagrad(W, S1, G, every, lr, eps)
    elif optimizer == "RMSprop":
        ref._rmsprop_dense_decay(W, S1, G, lr, dt(np.float32(0.9)), eps)
    elif optimizer == "Adamax":
        ref._adamax(W, S1, S2, G, every, dt(float(lr) / (1.0 - float(b1) ** tt)), b1, b2, eps)
    else:
        ref._adam_dense_decay(W, S1, S2, G, dt(float(lr) * np.sqrt(1.0 - float(b2) ** tt) / (1.0 - float(b1) ** tt)), b1, b2, eps)
    return W, S1, S2


def removal_factors(c, optimizer, k4):
    """One float4 (index k4 of the stride's float4) of ONE list's contribution to ONE shared id left out of the sum, for every
    shared id and every list that names it: (by how many tolerances atol + rtol |w| the applied WEIGHT then moves — the
    largest of the float4's model columns —, the same over the weight and the optimizer's slots), one value per removal."""
    G, _, count, _ = dense_reference(c)
    cols = np.arange(4 * k4, min(4 * k4 + 4, c.dm))
    t = seeded_tables(c.V, c.dm, optimizer)
    slots = ("M_", "V_") if optimizer in ("Adam", "Adamax") else ("A_", None)
    weight, any_ = [], []
    for l in c.lists:
        for s, name in ((0, "R"), (1, "C")):
            sel = (l["sides"] == s) & (count[s][l["ids"]] >= 2)
            ids = l["ids"][sel]
            if not len(ids):
                continue
            W = getattr(t, name)[np.ix_(ids, cols)]
            S1 = getattr(t, slots[0] + name)[np.ix_(ids, cols)]
            S2 = getattr(t, slots[1] + name)[np.ix_(ids, cols)] if slots[1] else None
            whole = G[s][np.ix_(ids, cols)]
            less = whole - l["entries"][sel][:, cols].astype(np.float64)
            a, b = updated(optimizer, W, S1, S2, whole), updated(optimizer, W, S1, S2, less)
            moved = [np.abs(x - y) / ((1e-9 if optimizer == "Adam" and i == 2 else ATOL) + RTOL * np.abs(x))
                     for i, (x, y) in enumerate(zip(a, b)) if x is not None]
            weight.append(moved[0].max(axis=1))
            any_.append(np.max(moved, axis=0).max(axis=1))
    return np.concatenate(weight), np.concatenate(any_)


# ---- the long lists: more entries than one grid sweep of apply_packed_kernel has lane groups
def lane_groups(dm_stride):
    """T: the most lane groups a launch of the exchange kernels has at this row stride, kMaxBlocks (kBlock / LPR)."""
    return kMaxBlocks * (kBlock // pick_row_shape(dm_stride // 4)[0])


def long_counts(stride):
    """The entry counts of the four lists of the long case: 3T + 2, 2T + 1, 2T and T.  apply_packed_kernel's grid is sized by the
    longest list of a launch and capped at T lane groups, so group gg of list k holds the entries gg, gg + T, gg + 2T, ..."""
    T = lane_groups(stride)
    return (3 * T + 2, 2 * T + 1, 2 * T, T)


def entries_per_group(n, T):
    """How many entries each of the T lane groups holds of a list of n entries: int64[T]."""
    return (n - np.arange(T) + T - 1) // T


def long_case(stride):
    """Four bare lists of long_counts(stride) entries over 2T + 41 ids a side: the longest names three quarters of a side, the
    others a half, a half and a quarter, drawn at random — ids named by none, one and several lists are all plentiful."""
    rng = np.random.default_rng(7 + stride)
    T = lane_groups(stride)
    V_side = 2 * T + 41
    lists = []
    for n in long_counts(stride):
        n_row = (n + 1) // 2
        ids = np.concatenate([rng.permutation(V_side)[:n_row], rng.permutation(V_side)[:n - n_row]]).astype(np.int32)
        sds = np.concatenate([np.zeros(n_row, np.int8), np.ones(n - n_row, np.int8)])
        e = np.zeros((n, stride + 4), np.float32)
        e[:, :stride] = _levels(rng, n, stride)
        e[:, stride] = _levels(rng, n)
        e.view(np.int32)[:, stride + 1] = ids
        e.view(np.int32)[:, stride + 2] = sds
        lists.append(dict(kind="bare", entries=e, ids=ids, sides=sds, partials=None, fixed_side=-1))
    return PackedCase(stride, stride, tuple(lists), V_side, 0)
