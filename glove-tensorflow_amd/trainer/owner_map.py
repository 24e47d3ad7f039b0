"""Frequency-balanced row ownership for the sharded multi-GPU forms, as a relabelling of the vocabulary.

The sharded forms place id u on rank u % world at local index u // world (trainer.stepper.owned_rows).  Vocabulary ids are
sorted by count, so under that rule rank 0 owns the heaviest id of every residue class and `route_by_row_owner` hands it
far more nonzeros than the last rank receives (Zipf(1.0), V = 400 k, 8 ranks: 1.69 x).  Every rank cycles through its own
epochs at a fixed local batch, so the nonzeros of the light ranks are revisited that much more often: the objective is
re-weighted.

`balanced_relabel` returns a bijection `perm` of [0, V): id u is renamed perm[u] before anything else sees it, and the
ownership rule stays what it is — perm[u] % world owns, perm[u] // world is the local index.  The stepper, the routing, the
owner-major col numbering and every kernel keep their arithmetic; only the stream (NonzeroStream(relabel=)) and the
whole-table reads and writes (DeviceTables.gathered_state_dict / load_whole_state_dict) know about the map.  It is a pure
function of the row histogram: every rank computes it locally, nothing of it is stored in a checkpoint.
"""
from __future__ import annotations

import heapq

import numpy as np

HEAD = 8192         # ids placed one by one; Zipf(1.0): the ids behind them hold < 1 / 8192 of the heaviest id's mass each


def owned_rows(V: int, world: int, rank: int) -> int:
    """trainer.stepper.owned_rows (restated: this module imports nothing of the trainer)."""
    return (V - rank + world - 1) // world


def balanced_relabel(counts, world: int, head: int = HEAD) -> np.ndarray:
    """perm: int64[V], a bijection of [0, V) under which the ranks' shares of `counts` are as equal as the cardinality
    constraint allows: rank r must receive exactly owned_rows(V, world, r) ids, or perm % world would not be the ownership
    the tables are cut by.

    Ids in descending count (stable: ties keep the lower id first).  The first `head` of them go one by one to the rank with
    the smallest load so far that still has room (ties: the lower rank); the rest are dealt in a snake — the ranks lightest
    first, then that order reversed, and again — for as long as every rank has room; the last few go to the lightest rank
    with room.  local[u] is u's order of arrival on its rank, perm[u] = local[u] * world + owner[u].
    Deterministic: the same arguments give the same array on every rank."""
    counts = np.asarray(counts, dtype=np.int64)
    V, world = len(counts), int(world)
    if world < 1:
        raise ValueError("world must be positive, got %d" % world)
    order = np.argsort(-counts, kind="stable")
    cap = [owned_rows(V, world, r) for r in range(world)]
    load, seats = [0] * world, [0] * world
    owner = np.empty(V, dtype=np.int64)
    local = np.empty(V, dtype=np.int64)

    def seat(u, r):
        owner[u], local[u] = r, seats[r]
        seats[r] += 1
        load[r] += int(counts[u])

    # ---- head: greedy, on a heap of (load, rank); a full rank leaves the heap for good
    n_head = min(int(head), V)
    heap = [(0, r) for r in range(world) if cap[r] > 0]
    heapq.heapify(heap)
    for u in order[:n_head].tolist():
        _, r = heapq.heappop(heap)
        seat(u, r)
        if seats[r] < cap[r]:
            heapq.heappush(heap, (load[r], r))
    # ---- tail: whole rounds of the snake while every rank has room
    tail = order[n_head:]
    rounds = min(cap[r] - seats[r] for r in range(world))
    lightest_first = np.argsort(np.asarray(load), kind="stable")
    pattern = np.concatenate([lightest_first, lightest_first[::-1]])
    dealt = np.tile(pattern, rounds // 2 + 1)[:rounds * world]
    ids = tail[:len(dealt)]
    owner[ids] = dealt
    for r in range(world):
        got = ids[dealt == r]
        local[got] = seats[r] + np.arange(len(got))
        seats[r] += len(got)
        load[r] += int(counts[got].sum())
    # ---- the rest (fewer than the head held: the ranks' seat counts differ by what the head gave them)
    for u in tail[len(dealt):].tolist():
        seat(u, min((r for r in range(world) if seats[r] < cap[r]), key=lambda r: (load[r], r)))
    return local * world + owner


def inverse(perm) -> np.ndarray:
    """inv[perm[u]] = u: the token whose rows sit at relabelled id p is inv[p]."""
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm), dtype=np.int64)
    return inv


def shard_loads(counts, perm, world: int) -> np.ndarray:
    """int64[world]: what each rank receives of `counts` when id u lives on rank perm[u] % world (exact integer sums).
    perm = None: the plain rule u % world."""
    counts = np.asarray(counts, dtype=np.int64)
    ids = np.arange(len(counts), dtype=np.int64) if perm is None else np.asarray(perm, dtype=np.int64)
    owner = ids % int(world)
    return np.asarray([counts[owner == r].sum() for r in range(int(world))], dtype=np.int64)


def imbalance(loads) -> float:
    """most / least of a load vector (an empty rank counts as one nonzero, as NonzeroStream's log line does)."""
    loads = np.asarray(loads, dtype=np.int64)
    return float(loads.max()) / float(max(int(loads.min()), 1))


def id_histogram(ids, V: int, dist=None) -> np.ndarray:
    """int64[V]: how many entries of `ids` (a numpy array or a tensor on any device) name each id, ids outside [0, V)
    counted as id 0 (the unknown token) the way the stream clamps them.  `dist`: the entries are this rank's part of the
    stream (a presharded one): one all-reduce makes the histogram the whole stream's (collective)."""
    import torch
    t = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(ids))
    t = t.long()
    t = torch.where((t < 0) | (t >= V), torch.zeros_like(t), t)
    hist = torch.bincount(t, minlength=int(V))
    if dist is not None:
        dist.all_reduce(hist)
    return hist.cpu().numpy().astype(np.int64)
