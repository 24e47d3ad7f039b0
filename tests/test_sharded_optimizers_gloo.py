"""The sharded multi-GPU forms under every Keras optimizer, on CPU: world_size 2 over gloo, kernels replaced by the oracle
(tests/sharded_oracle_backend.py).

Property under test, the one the Adagrad forms are held to in tests/test_dp_gloo.py: N ranks, each stepping on the nonzeros
routed to the owner of their rows with inv_batch = 1 / (N B), equal one rank stepping on the union of the batches under the
same optimizer (glove_ref.train_step) — weights, every slot, the global bias with its slots, global_step."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent / "oracle"))
from helpers import free_port  # noqa: E402

WORLD = 2
B, V, D, STEPS = 96, 40, 8, 5
OPTIMIZERS = ("Adagrad", "SGD", "RMSprop", "Adamax", "Adam", "Adadelta", "Ftrl", "Nadam")
ROW_SIDE = ("R", "br")
COL_SIDE = ("C", "bc")
PREFIXES = ("", "A_", "M_", "V_", "U_", "Z_")
SCALARS = ("g", "A_g", "M_g", "V_g", "U_g", "Z_g", "m_cache")


def _batches():
    from helpers import make_batch                       # Zipf ids on both sides (the head ids land on both ranks' lists)
    return [[make_batch(100 * s + r, B, V) for r in range(WORLD)] for s in range(STEPS)]


def _hyper(optimizer):
    kw = dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.05)
    if optimizer == "SGD":
        kw.update(momentum=0.9, nesterov=True)
    return kw


def _worker(rank, port, out_dir, optimizer, form):
    for p in (HERE.parent, HERE.parent / "oracle", HERE):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    import glove_ref as ref
    from oracle_backend import OracleTables
    from sharded_oracle_backend import ShardedOracleBackend
    from trainer.stepper import RowShardedStepper, ShardedStepper, route_by_row_owner
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    full = ref.Tables(V, D, optimizer, dtype=np.float64, seed=3)
    shard = full.copy()
    cut = ROW_SIDE + (COL_SIDE if form == "both" else ())
    for n in cut:                                    # id % world == rank, local index id // world: the variable and its slots
        for p in PREFIXES:
            if hasattr(full, p + n):
                setattr(shard, p + n, getattr(full, p + n)[rank::WORLD].copy())
    tables = OracleTables(shard)
    backend = ShardedOracleBackend()
    kw = _hyper(optimizer)
    if form == "both":
        stepper = ShardedStepper(backend, tables, kw, B, WORLD, rank, dist)
    else:
        stepper = RowShardedStepper(backend, tables, kw, B, WORLD, dist, exchange=form)
    items = []
    for step_batches in _batches():
        mine = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in zip(("row", "col", "w", "y"), step_batches[rank])}
        routed = route_by_row_owner(mine, WORLD, rank, dist)
        if form == "both":
            items.append(stepper.add_batch(routed["row"], routed["col"], routed["w"], routed["y"], 32))
        else:
            items.append(backend.build_plan(*(routed[k].numpy() for k in ("row", "col", "w", "y")), V, 32))
    if form != "both":
        stepper.prepare(items)
        assert stepper.rows == (form == "rows")
    for it in items:
        stepper.step(it)
    out = {k: v for k, v in vars(shard).items() if isinstance(v, np.ndarray)}
    out.update({a: np.asarray(getattr(shard, a)) for a in SCALARS + ("step",) if hasattr(shard, a)})
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def _joint(optimizer):
    import glove_ref as ref
    t = ref.Tables(V, D, optimizer, dtype=np.float64, seed=3)
    hp = ref.Hyper(**_hyper(optimizer))
    for step_batches in _batches():
        ref.train_step(t, *[np.concatenate([b[i] for b in step_batches]) for i in range(4)], hp)
    return t


CASES = [(o, f) for o in OPTIMIZERS for f in ("dense", "rows", "both")
         if not (f == "dense" and o in ("SGD", "Adamax", "Adadelta", "Ftrl", "Nadam"))]


@pytest.mark.parametrize("optimizer,form", CASES)
def test_sharded_step_equals_single_rank_on_the_joint_batch(tmp_path, optimizer, form):
    mp.spawn(_worker, args=(free_port(), str(tmp_path), optimizer, form), nprocs=WORLD, join=True)
    t = _joint(optimizer)
    shards = [dict(np.load(tmp_path / ("rank%d.npz" % r))) for r in range(WORLD)]
    cut = ROW_SIDE + (COL_SIDE if form == "both" else ())
    checked = 0
    for r, s in enumerate(shards):
        for n in ROW_SIDE + COL_SIDE:
            for p in PREFIXES:
                if not hasattr(t, p + n):
                    continue
                want = getattr(t, p + n)[r::WORLD] if n in cut else getattr(t, p + n)
                np.testing.assert_allclose(s[p + n], want, rtol=1e-10, atol=1e-13, err_msg="rank %d %s" % (r, p + n))
                checked += 1
        for a in SCALARS:
            if hasattr(t, a):
                np.testing.assert_allclose(s[a], getattr(t, a), rtol=1e-10, atol=1e-13, err_msg="rank %d %s" % (r, a))
        assert int(s["step"]) == STEPS
    # every variable and every slot was compared (Adam: w, m, v of four variables on both ranks)
    assert checked == WORLD * 4 * sum(hasattr(t, p + "R") for p in PREFIXES)


@pytest.mark.parametrize("optimizer", ["SGD", "Adamax", "Adadelta", "Ftrl", "Nadam"])
def test_touched_rows_optimizers_refuse_the_dense_col_exchange(optimizer):
    """Only touched rows move under them: the col side needs the ranks' lists (the union of their ids), as in Stepper."""
    import glove_ref as ref
    from oracle_backend import OracleTables
    from sharded_oracle_backend import ShardedOracleBackend
    from trainer.stepper import RowShardedStepper
    tables = OracleTables(ref.Tables(V, D, optimizer, dtype=np.float64, seed=3))

    class _Dist:                     # never reached: the constructor decides before any collective
        pass
    with pytest.raises(ValueError, match="touched-rows exchange"):
        RowShardedStepper(ShardedOracleBackend(), tables, _hyper(optimizer), B, WORLD, _Dist(), exchange="dense")
    s = RowShardedStepper(ShardedOracleBackend(), tables, _hyper(optimizer), B, WORLD, _Dist(), exchange="auto")
    assert s.exchange == "rows"


def test_unknown_optimizer_names_are_refused():
    from types import SimpleNamespace
    from trainer.stepper import RowShardedStepper
    tables = SimpleNamespace(optimizer="Lion", device=torch.device("cpu"))
    with pytest.raises(ValueError, match="eight Keras names"):
        RowShardedStepper(None, tables, {}, B, WORLD, None)


# ---- both tables sharded under reshuffled epochs (col ids numbered owner-major, as the trainer's --shard-cols runs)
RB, RN, RSTEPS = 40, 403, 24            # ~200 routed pairs per rank -> 5 batches per epoch: 24 steps cross four epoch boundaries


def _reshuffle_worker(rank, port, out_dir, optimizer):
    for p in (HERE.parent, HERE.parent / "oracle", HERE):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    import glove_ref as ref
    from helpers import zipf_ids
    from oracle_backend import OracleTables
    from sharded_oracle_backend import ShardedOracleBackend
    from trainer.data_utils import NonzeroStream
    from trainer.stepper import ReshufflingRunner, ShardedStepper
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    rng = np.random.default_rng(0)
    row, col = zipf_ids(rng, RN, V), zipf_ids(rng, RN, V)
    col[row == col] = (col[row == col] + 1) % V
    coo = dict(row=row, col=col, w=rng.uniform(0.1, 1.0, RN).astype(np.float32), y=rng.normal(size=RN).astype(np.float32))
    full = ref.Tables(V, D, optimizer, dtype=np.float64, seed=3)
    shard = full.copy()
    for n in ROW_SIDE + COL_SIDE:
        for p in PREFIXES:
            if hasattr(full, p + n):
                setattr(shard, p + n, getattr(full, p + n)[rank::WORLD].copy())
    tables = OracleTables(shard)
    backend = ShardedOracleBackend()
    stream = NonzeroStream(coo, RB, V, backend, "cpu", rank=rank, world=WORLD, seed=11, static_plans=False, route=dist,
                           cols_by_owner=WORLD)
    seen = []

    class Recording(ShardedStepper):          # the batches in the order the epochs prepare them = the order they are stepped
        def add_batch(self, row, col, w, y, chunk_cap=0):
            seen.append(tuple(np.asarray(a).copy() for a in (row, col, w, y)))
            return super().add_batch(row, col, w, y, chunk_cap)

    stepper = Recording(backend, tables, _hyper(optimizer), RB, WORLD, rank, dist)
    runner = ReshufflingRunner(None, stream, tables, stepper.hyper, chunk_cap=8, burst=7, stepper=stepper)
    assert stepper.col_per == stream.col_per > 0
    done = 0
    while done < RSTEPS:
        done += runner.run(min(3, RSTEPS - done))
    per = stream.col_per
    out = {k: v for k, v in vars(shard).items() if isinstance(v, np.ndarray)}
    out.update({a: np.asarray(getattr(shard, a)) for a in SCALARS + ("step",) if hasattr(shard, a)})
    for s, (r, c, w, y) in enumerate(seen[:RSTEPS]):
        # global ids: row u of this rank's shard is u * world + rank; owner-major col id c is (c % per) * world + c // per
        out.update({"b%d_row" % s: r.astype(np.int64) * WORLD + rank, "b%d_col" % s: (c % per) * WORLD + c // per,
                    "b%d_w" % s: w, "b%d_y" % s: y})
    out["bpe"] = np.asarray(runner.nb)
    np.savez(os.path.join(out_dir, "re%d.npz" % rank), **out)
    dist.destroy_process_group()


def test_reshuffled_epochs_with_both_tables_sharded_under_adam(tmp_path):
    """ShardedStepper under the reshuffling runner with Adam: epochs re-dealt, each epoch's fetch lists prepared when it starts,
    owner-major col ids — equal to the oracle stepping on the ranks' joint batch, step by step, across four epoch boundaries."""
    import glove_ref as ref
    mp.spawn(_reshuffle_worker, args=(free_port(), str(tmp_path), "Adam"), nprocs=WORLD, join=True)
    ranks = [dict(np.load(tmp_path / ("re%d.npz" % r))) for r in range(WORLD)]
    assert int(ranks[0]["bpe"]) * 4 < RSTEPS
    t = ref.Tables(V, D, "Adam", dtype=np.float64, seed=3)
    hp = ref.Hyper(**_hyper("Adam"))
    for s in range(RSTEPS):
        ref.train_step(t, *[np.concatenate([rk["b%d_%s" % (s, k)] for rk in ranks]) for k in ("row", "col", "w", "y")], hp)
    for r, rk in enumerate(ranks):
        for n in ROW_SIDE + COL_SIDE:
            for p in ("", "M_", "V_"):
                np.testing.assert_allclose(rk[p + n], getattr(t, p + n)[r::WORLD], rtol=1e-10, atol=1e-13, err_msg=p + n)
        for a in ("g", "M_g", "V_g"):
            np.testing.assert_allclose(rk[a], getattr(t, a), rtol=1e-10, atol=1e-13, err_msg=a)
        assert int(rk["step"]) == RSTEPS
