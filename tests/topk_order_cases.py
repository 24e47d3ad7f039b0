"""TEST-ONLY generator of the cases of tests/test_gpu_topk_order.py: vocabularies whose top-k order is decided by exact
ties, and the ranking tf.math.top_k gives on them (larger score first, ties to the lower id), in float64 NumPy.

A vocabulary is G prototype rows (Gaussian, d = 16, float32), each copied to many ids: group_of[v] is the prototype of
row v, laid out by a seeded permutation of [0, V).  Bit-identical rows get bit-identical scores from any kernel that
does the same arithmetic on the same operands, so the order inside a group is decided by the id alone, in every
register, lane, wave, segment and stage of the selection.  Between groups the float64 scores of every query differ by
GROUP_GAP at least (1e-4: ten times the GAP of tests/test_gpu_analogy.py, a hundred times the score atol; for 3CosMul,
whose scores exceed 1, by GROUP_GAP max(1, |s|)): float32 rounding cannot reorder two groups.  Prototypes and questions
are drawn by rejection until that holds, and build() asserts it.  The expected ids are therefore
lexsort(score descending, id ascending) with no position left out.

Never imported by the product."""
import dataclasses
import functools

import numpy as np

D = 16
GROUP_GAP = 1e-4
EPS_NORM = 1e-12                # tf.math.l2_normalize's clamp
COSMUL_EPS = 1e-3
PATHS = ("predict", "cosadd", "cosmul")


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    V: int
    n: int
    k_predict: int              # 0: the path is not run on this case
    k_analogy: int
    groups: int = 40
    dead: tuple = ()            # (id, "nan" | "inf"): rows made non-finite after the layout (predict path only)

    def k(self, path):
        return self.k_predict if path == "predict" else self.k_analogy


# ceil(V / 4096) segments of the first stage; a later stage has ceil(segments k / 4096)
SPECS = (
    Spec("tail_of_4", 4100, 130, 1024, 1024),           # last segment: 4 candidates, 1,020 empty slots; k at its maximum; two stages
    Spec("three_stages", 16388, 3, 1024, 1024),         # 5 -> 2 -> 1 segments: both ping-pong buffers are source and destination
    Spec("tail_of_1", 12289, 130, 20, 20),              # last segment: one candidate; two query tiles
    Spec("all_identical", 5000, 6, 100, 100, groups=1),  # one float for every score
    Spec("whole_vocabulary", 1024, 8, 1024, 1021),      # the ranking is one permutation of the vocabulary
    Spec("k_1", 4100, 130, 1, 1),
    Spec("V_1", 1, 1, 1, 0, groups=1),
    Spec("V_4", 4, 4, 0, 1, groups=4),
    # non-finite rows (predict): never returned; k up to the number of finite rows
    Spec("dead_rows", 4100, 16, 1024, 0, dead=((4098, "nan"), (17, "inf"))),
    Spec("dead_rows_all_finite_taken", 1024, 8, 1022, 0, dead=((1023, "nan"), (0, "inf"))),
)
BY_NAME = {s.name: s for s in SPECS}


def unit_rows(P):
    P = np.asarray(P, np.float64)
    return P / np.sqrt(np.maximum((P * P).sum(1, keepdims=True), EPS_NORM))


def group_scores(P, path, q):
    """float64 scores [n, G] of every prototype for the queries q: prototype ids [n] (predict) or [n, 3] = (a, b, c)."""
    u = unit_rows(P)
    q = np.asarray(q, np.int64)
    if path == "predict":
        return u[q] @ u.T
    if path == "cosadd":
        x = u[q[:, 1]] - u[q[:, 0]] + u[q[:, 2]]
        return (x @ u.T) / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), EPS_NORM))
    sa, sb, sc = ((1.0 + np.clip(u[q[:, j]] @ u.T, -1, 1)) * 0.5 for j in range(3))
    return sb * sc / (sa + COSMUL_EPS)


def smallest_gap(s, relative=False):
    """The smallest distance of two groups' scores over all queries (relative: in units of max(1, |score|))."""
    if s.shape[1] < 2:
        return np.inf
    o = np.sort(s, axis=1)
    gap = o[:, 1:] - o[:, :-1]
    if relative:
        gap = gap / np.maximum(1.0, np.maximum(np.abs(o[:, 1:]), np.abs(o[:, :-1])))
    return float(gap.min())


def question_ok(P, g3):
    g3 = np.asarray(g3).reshape(1, 3)
    return (smallest_gap(group_scores(P, "cosadd", g3)) >= GROUP_GAP and
            smallest_gap(group_scores(P, "cosmul", g3), relative=True) >= GROUP_GAP)


def prototypes(rng, G):
    """G float32 rows whose pairwise cosines, as seen from every row, are GROUP_GAP apart: drawn one at a time."""
    P = np.zeros((0, D), np.float32)
    while len(P) < G:
        cand = np.concatenate([P, rng.standard_normal((1, D)).astype(np.float32)])
        if smallest_gap(group_scores(cand, "predict", np.arange(len(cand)))) >= GROUP_GAP:
            P = cand
    return P


def edge_ids(V):
    """Ids on the edges of the query tiles, vocabulary tiles and selection segments."""
    e = [0, 127, 128, V - 1] + [x for s in range(4096, V, 4096) for x in (s - 1, s)]
    return [x for x in dict.fromkeys(e) if 0 <= x < V]


@functools.lru_cache(maxsize=None)
def build(name):
    """dict of a case: W [V, 16] float32, group_of [V], P (prototypes), queries [n] int32, abc [n, 3] int32 (None where
    the path is not run).  Computed once, shared, never written to."""
    spec = BY_NAME[name]
    rng = np.random.default_rng(7000 + spec.V + spec.groups + len(spec.dead))
    G, V, n = min(spec.groups, spec.V), spec.V, spec.n
    P = prototypes(rng, G)
    group_of = np.empty(V, np.int64)
    group_of[rng.permutation(V)] = np.arange(V) % G
    W = P[group_of].copy()
    dead = np.array([v for v, _ in spec.dead], np.int64)
    queries = abc = None
    if spec.k_predict:
        queries = rng.integers(0, V, n)
        edges = [e for e in edge_ids(V) if e not in dead][:n]
        queries[:len(edges)] = edges
        for i in np.flatnonzero(np.isin(queries, dead)):     # finite queries only
            queries[i] = next(v for v in range(V) if v not in dead)
        queries = queries.astype(np.int32)
    if spec.k_analogy:
        abc = np.empty((n, 3), np.int32)
        edges = edge_ids(V)
        for i in range(n):
            while True:
                q = rng.choice(V, 3, replace=False)
                if i < len(edges) and V > 4:                 # the first questions sit on the edges, in turn as a, b and c
                    if edges[i] in q[1:]:
                        continue
                    q[0] = edges[i]
                    q = np.roll(q, i % 3)
                if G == 1 or question_ok(P, group_of[q]):
                    abc[i] = q
                    break
        if name == "all_identical":                          # questions that take ids out of the first k
            abc[:4] = [[0, 1, 2], [5, 50, 99], [4999, 4096, 4095], [100, 3, 200]]
        assert all(len(set(q)) == 3 for q in abc.tolist())
    for v, kind in spec.dead:
        if kind == "nan":
            W[v] = np.nan
        else:
            W[v, 3] = np.inf
    out = {"spec": spec, "W": W, "P": P, "group_of": group_of, "queries": queries, "abc": abc, "dead": dead}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def scores_full(case, path):
    """float64 scores [n, V]: a group's score at every id of the group; -inf at a question's own three ids and at the
    non-finite rows."""
    spec = case["spec"]
    if path == "predict":
        q = case["group_of"][case["queries"]]
    else:
        q = case["group_of"][case["abc"]]
    sg = group_scores(case["P"], path, q)
    if sg.shape[1] > 1:
        gap = smallest_gap(sg, relative=(path == "cosmul"))
        assert gap >= GROUP_GAP, (spec.name, path, gap)
    s = sg[:, case["group_of"]]
    if path != "predict":
        rows = np.arange(len(s))
        for j in range(3):
            s[rows, case["abc"][:, j]] = -np.inf
    s[:, case["dead"]] = -np.inf
    return s


@functools.lru_cache(maxsize=None)
def expected(name, path):
    """(scores [n, k] float64, ids [n, k] int32) in the order of tf.math.top_k: lexsort by (score descending, id
    ascending).  Every position is exact: none is left out of the comparison."""
    case = build(name)
    k = case["spec"].k(path)
    assert k > 0
    s = scores_full(case, path)
    ids = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    order = np.stack([np.lexsort((ids[i], -s[i]))[:k] for i in range(len(s))])
    want_s = np.take_along_axis(s, order, 1)
    assert np.isfinite(want_s).all()                         # k never reaches an excluded or non-finite row
    want_s.setflags(write=False)
    order = order.astype(np.int32)
    order.setflags(write=False)
    return want_s, order


def runs(name):
    """The paths a case runs."""
    spec = BY_NAME[name]
    return [p for p in PATHS if spec.k(p)]
