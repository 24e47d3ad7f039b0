"""RowWiseAdagrad on the multi-GPU forms, on CPU: world_size 2 over gloo, kernels replaced by the float64 restatement
(tests/rowwise_oracle_backend.py), Zipf ids — the set-up and the tolerances of tests/test_sharded_optimizers_gloo.py.

Property under test: two ranks — data parallel on the touched-rows exchange, row table sharded, both tables sharded — equal one
rank stepping on the joint batch (rowwise_adagrad_ref.train_step): weights, the accumulators (one float per row on all four
variables: a shard's are cut by row), the global bias with its accumulator, global_step.  The square is of the SUM of the
ranks' gradient rows of an id: a form that accumulated per rank would miss the cross terms and fail here."""
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
from test_sharded_optimizers_gloo import B, COL_SIDE, D, ROW_SIDE, STEPS, V, WORLD, _batches, _hyper  # noqa: E402

PREFIXES = ("", "A_")
SCALARS = ("g", "A_g")


def _worker(rank, port, out_dir, form):
    for p in (HERE.parent, HERE.parent / "oracle", HERE):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    import rowwise_adagrad_ref as rw
    from rowwise_oracle_backend import RowWiseOracleBackend
    from oracle_backend import OracleTables
    from trainer.stepper import RowShardedStepper, ShardedStepper, Stepper, route_by_row_owner
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    full = rw.tables(V, D, seed=3)
    shard = full.copy()
    cut = () if form == "dp" else ROW_SIDE + (COL_SIDE if form == "both" else ())
    for n in cut:                                    # id % world == rank, local index id // world: the variable and its accumulator(s)
        for p in PREFIXES:
            setattr(shard, p + n, getattr(full, p + n)[rank::WORLD].copy())
    tables = OracleTables(shard)
    assert tables.optimizer == "RowWiseAdagrad" and shard.A_R.ndim == shard.A_C.ndim == 1 and len(shard.A_R) == len(shard.R)
    backend = RowWiseOracleBackend()
    kw = _hyper("RowWiseAdagrad")
    if form == "dp":
        stepper = Stepper(backend, tables, dict(kw, optimizer="RowWiseAdagrad"), B, WORLD, dist, exchange="auto")
        assert stepper.exchange == "rows"
    elif form == "both":
        stepper = ShardedStepper(backend, tables, kw, B, WORLD, rank, dist)
    else:
        stepper = RowShardedStepper(backend, tables, kw, B, WORLD, dist, exchange="auto")
        assert stepper.exchange == "rows"
    items = []
    for step_batches in _batches():
        if form == "dp":
            items.append(backend.build_plan(*step_batches[rank], V, 32))
            continue
        mine = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in zip(("row", "col", "w", "y"), step_batches[rank])}
        routed = route_by_row_owner(mine, WORLD, rank, dist)
        if form == "both":
            items.append(stepper.add_batch(routed["row"], routed["col"], routed["w"], routed["y"], 32))
        else:
            items.append(backend.build_plan(*(routed[k].numpy() for k in ("row", "col", "w", "y")), V, 32))
    if form != "both":
        stepper.prepare(items)
        assert stepper.rows
    for it in items:
        stepper.step(it)
    out = {k: v for k, v in vars(shard).items() if isinstance(v, np.ndarray)}
    out.update({a: np.asarray(getattr(shard, a)) for a in SCALARS + ("step",)})
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def joint():
    """The restatement stepping on the ranks' joint batches: computed once, read by every form."""
    import glove_ref as ref
    import rowwise_adagrad_ref as rw
    t = rw.tables(V, D, seed=3)
    hp = ref.Hyper(**_hyper("RowWiseAdagrad"))
    for step_batches in _batches():
        rw.train_step(t, *[np.concatenate([b[i] for b in step_batches]) for i in range(4)], hp)
    return t


@pytest.mark.parametrize("form", ["dp", "rows", "both"])
def test_two_ranks_equal_the_restatement_on_the_joint_batch(tmp_path, joint, form):
    mp.spawn(_worker, args=(free_port(), str(tmp_path), form), nprocs=WORLD, join=True)
    t = joint
    shards = [dict(np.load(tmp_path / ("rank%d.npz" % r))) for r in range(WORLD)]
    cut = () if form == "dp" else ROW_SIDE + (COL_SIDE if form == "both" else ())
    for r, s in enumerate(shards):
        for n in ROW_SIDE + COL_SIDE:
            for p in PREFIXES:
                want = getattr(t, p + n)[r::WORLD] if n in cut else getattr(t, p + n)
                np.testing.assert_allclose(s[p + n], want, rtol=1e-10, atol=1e-13, err_msg="rank %d %s" % (r, p + n))
        for a in SCALARS:
            np.testing.assert_allclose(s[a], getattr(t, a), rtol=1e-10, atol=1e-13, err_msg="rank %d %s" % (r, a))
        assert int(s["step"]) == STEPS
    if form == "dp":
        for k in shards[0]:
            np.testing.assert_array_equal(shards[0][k], shards[1][k], err_msg=k)         # replicas stay identical
