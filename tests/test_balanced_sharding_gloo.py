"""--shard-balance frequency on CPU: world_size 2 over gloo, kernels replaced by the float64 oracle (as tests/test_dp_gloo.py
spawns its workers; ids drawn Zipf(1.0)).

The ids of the stream are renamed by trainer.owner_map.balanced_relabel before anything else sees them and the ranks hold
their tables in the renamed order; everything a user addresses by vocabulary id — checkpoints, the gathered model — stays in
vocabulary order.  Property under test: two ranks on renamed ids == one rank of the oracle stepping on the joint batch in
ORIGINAL ids, and a checkpoint of such a run is the checkpoint of any other run."""
import json
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
from helpers import SLOTS, free_port  # noqa: E402
from test_dp_gloo import B, D, V, WORLD, _batches, _fully_sharded_batches  # noqa: E402

RTOL, ATOL = 1e-10, 1e-13                  # tests/test_dp_gloo.py's
NAMES = ("R", "C", "br", "bc")
GOLDEN = HERE / "golden"


def _enter(rank, port):
    for p in (HERE.parent, HERE.parent / "oracle", HERE):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)


def _hyper(optimizer):
    return dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.05, optimizer=optimizer)


def _map_of(step_batches_list):
    """The map of a run over these per-step, per-rank batches: the row histogram of the whole stream of all ranks."""
    from trainer.owner_map import balanced_relabel, id_histogram
    rows = np.concatenate([b[0] for step in step_batches_list for b in step])
    counts = id_histogram(rows, V)
    return counts, balanced_relabel(counts, WORLD)


# ---- float64 DeviceTables on the CPU: the product's whole-model (de)serialisation around the oracle's arrays
def _f64_tables(optimizer, V_row=None, V_col=None):
    from trainer.hip_api import DeviceTables
    dt = DeviceTables(V, D, optimizer, device="cpu", seed=0, V_row=V_row, V_col=V_col)
    assert dt.d == D                                         # no alignment padding at this size
    for name in ("_R", "_C", "_br", "_bc"):
        setattr(dt, name, getattr(dt, name).double())
    dt.s1 = {n: x.double() for n, x in dt.s1.items()}
    dt.s2 = {n: x.double() for n, x in dt.s2.items()}
    return dt


def _whole_state(t):
    """A whole-model state dict, vocabulary order, of oracle tables (the format of DeviceTables.state_dict)."""
    sd = {"V": V, "d": D, "V_row": V, "optimizer": t.optimizer, "scalars": torch.zeros(8), "global_step": torch.tensor([t.step])}
    for n in NAMES:
        sd[n] = torch.from_numpy(getattr(t, n).copy())
        for k, pre in enumerate(SLOTS[t.optimizer]):
            sd["slot%d_%s" % (k + 1, n)] = torch.from_numpy(getattr(t, pre + n).copy())
    return sd


def _oracle_shard(full, dt):
    """The oracle tables of one rank: the arrays `dt` cut out of the whole model (copies), the scalars of `full`."""
    shard = full.copy()
    for n in NAMES:
        setattr(shard, n, getattr(dt, n).numpy().copy())
        for k, pre in enumerate(SLOTS[full.optimizer]):
            setattr(shard, pre + n, (dt.s1, dt.s2)[k][n].numpy().copy())
    return shard


def _put_back(dt, shard):
    for n in NAMES:
        getattr(dt, n).copy_(torch.from_numpy(getattr(shard, n)))
        for k, pre in enumerate(SLOTS[shard.optimizer]):
            (dt.s1, dt.s2)[k][n].copy_(torch.from_numpy(getattr(shard, pre + n)))


def _save_gathered(dt, shard, perm, path, rank, **more):
    """The ranks' shards gathered to vocabulary order through gathered_state_dict(relabel=) (collective); rank 0 writes."""
    _put_back(dt, shard)
    state = dt.gathered_state_dict(dist, WORLD, relabel=perm)
    if rank == 0:
        arrays = {k: v.numpy() for k, v in state.items() if torch.is_tensor(v) and k not in ("scalars", "global_step")}
        np.savez(path, g=np.asarray(shard.g), step=np.asarray(shard.step), **arrays, **more)


def _assert_equals_oracle(got, t, steps):
    for n in NAMES:
        assert got[n].shape == getattr(t, n).shape
        np.testing.assert_allclose(got[n], getattr(t, n), rtol=RTOL, atol=ATOL, err_msg=n)
        for k, pre in enumerate(SLOTS[t.optimizer]):
            np.testing.assert_allclose(got["slot%d_%s" % (k + 1, n)], getattr(t, pre + n), rtol=RTOL, atol=ATOL, err_msg=pre + n)
    np.testing.assert_allclose(got["g"], t.g, rtol=RTOL, atol=ATOL)
    assert int(got["step"]) == steps


# ---- 5. routing
RN_ROUTE = 1001


def _route_coo():
    from helpers import zipf_ids
    rng = np.random.default_rng(0)
    row, col = zipf_ids(rng, RN_ROUTE, V), zipf_ids(rng, RN_ROUTE, V)
    return dict(row=row, col=col, w=np.arange(RN_ROUTE, dtype=np.float32), y=rng.normal(size=RN_ROUTE).astype(np.float32))


def _routing_worker(rank, port, out_dir):
    _enter(rank, port)
    from oracle_backend import OracleBackend
    from trainer.data_utils import NonzeroStream
    from trainer.owner_map import balanced_relabel, id_histogram
    coo = _route_coo()
    perm = balanced_relabel(id_histogram(coo["row"], V), WORLD)
    st = NonzeroStream(coo, 50, V, OracleBackend(), "cpu", rank=rank, world=WORLD, seed=7, route=dist, relabel=perm)
    plain = NonzeroStream(coo, 50, V, OracleBackend(), "cpu", rank=rank, world=WORLD, seed=7, route=dist)
    assert not hasattr(plain, "col_imbalance") and st.col_imbalance >= 1.0
    np.savez(os.path.join(out_dir, "route%d.npz" % rank), w=st.w.numpy(), row=st.row.numpy(), col=st.col.numpy(), nnz=st.nnz,
             plain_nnz=plain.nnz, ratio=st.load_imbalance, plain_ratio=plain.load_imbalance)
    dist.destroy_process_group()


def test_every_nonzero_lands_on_the_rank_the_map_names(tmp_path):
    """Every nonzero on exactly one rank — the owner of its renamed row —, the ranks' totals exactly shard_loads(counts, perm),
    and most / least strictly below what id % world gives on the same data."""
    from trainer.owner_map import balanced_relabel, id_histogram, imbalance, inverse, shard_loads
    mp.spawn(_routing_worker, args=(free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    parts = [np.load(tmp_path / ("route%d.npz" % r)) for r in range(WORLD)]
    coo = _route_coo()
    counts = id_histogram(coo["row"], V)
    perm = balanced_relabel(counts, WORLD)
    serial = np.concatenate([p["w"] for p in parts])
    np.testing.assert_array_equal(np.sort(serial), np.arange(RN_ROUTE, dtype=np.float32))
    np.testing.assert_array_equal([int(p["nnz"]) for p in parts], shard_loads(counts, perm, WORLD))
    np.testing.assert_array_equal([int(p["plain_nnz"]) for p in parts], shard_loads(counts, None, WORLD))
    inv = inverse(perm)
    for r, p in enumerate(parts):           # local row u of rank r is renamed id u * world + r: the nonzero's own row and col
        which = p["w"].astype(np.int64)
        np.testing.assert_array_equal(inv[p["row"].astype(np.int64) * WORLD + r], coo["row"][which])
        np.testing.assert_array_equal(inv[p["col"]], coo["col"][which])
    balanced, modulo = imbalance(shard_loads(counts, perm, WORLD)), imbalance(shard_loads(counts, None, WORLD))
    print("most / least: %.4f balanced, %.4f id %% world" % (balanced, modulo))
    assert float(parts[0]["ratio"]) == balanced and float(parts[0]["plain_ratio"]) == modulo
    assert balanced < modulo


# ---- 6. per-step equality
def _step_worker(rank, port, out_dir, optimizer, form):
    _enter(rank, port)
    import glove_ref as ref
    from oracle_backend import OracleTables
    from sharded_oracle_backend import ShardedOracleBackend
    from trainer.stepper import RowShardedStepper, ShardedStepper, owned_rows, route_by_row_owner
    batches = _fully_sharded_batches() if form == "both" else _batches()
    _, perm = _map_of(batches)
    full = ref.Tables(V, D, optimizer, dtype=np.float64, seed=3)
    own = owned_rows(V, WORLD, rank)
    dt = _f64_tables(optimizer, V_row=own, V_col=own if form == "both" else None)
    dt.load_whole_state_dict(_whole_state(full), WORLD, rank, relabel=perm)       # vocabulary order, cut through the map
    shard = _oracle_shard(full, dt)
    tables = OracleTables(shard)
    backend = ShardedOracleBackend()
    if form == "both":
        stepper = ShardedStepper(backend, tables, _hyper(optimizer), B, WORLD, rank, dist)
    else:
        stepper = RowShardedStepper(backend, tables, _hyper(optimizer), B, WORLD, dist, exchange=form)
    items = []
    for step_batches in batches:
        row, col, w, y = step_batches[rank]
        mine = dict(row=torch.from_numpy(perm[row].astype(np.int32)), col=torch.from_numpy(perm[col].astype(np.int32)),
                    w=torch.from_numpy(np.ascontiguousarray(w)), y=torch.from_numpy(np.ascontiguousarray(y)))
        routed = route_by_row_owner(mine, WORLD, rank, dist)
        if form == "both":
            items.append(stepper.add_batch(routed["row"], routed["col"], routed["w"], routed["y"], 32))
        else:
            items.append(backend.build_plan(*(routed[k].numpy() for k in ("row", "col", "w", "y")), V, 32))
    if form != "both":
        stepper.prepare(items)
    for it in items:
        stepper.step(it)
    _save_gathered(dt, shard, perm, os.path.join(out_dir, "gathered.npz"), rank)
    dist.destroy_process_group()


@pytest.mark.parametrize("optimizer", ["Adagrad", "Adam"])
@pytest.mark.parametrize("form", ["dense", "rows", "both"])
def test_balanced_sharded_step_equals_single_rank_on_the_joint_batch_in_original_ids(tmp_path, optimizer, form):
    """The row-sharded step (dense col exchange, lists) and the both-tables-sharded step on renamed ids, the shards gathered
    to vocabulary order: the single-rank oracle stepping on the joint batch in original ids — weights and every slot."""
    import glove_ref as ref
    mp.spawn(_step_worker, args=(free_port(), str(tmp_path), optimizer, form), nprocs=WORLD, join=True)
    batches = _fully_sharded_batches() if form == "both" else _batches()
    _, perm = _map_of(batches)
    assert not np.array_equal(perm, np.arange(V))            # the map renames something
    t = ref.Tables(V, D, optimizer, dtype=np.float64, seed=3)
    hp = ref.Hyper(learning_rate=0.05)
    for step_batches in batches:
        ref.train_step(t, *[np.concatenate([b[i] for b in step_batches]) for i in range(4)], hp)
    _assert_equals_oracle(np.load(tmp_path / "gathered.npz"), t, len(batches))


# ---- 7. reshuffled epochs with both tables sharded
RB, RN, RSTEPS = 40, 403, 24            # ~200 routed pairs per rank -> 5 batches per epoch: 24 steps cross four epoch boundaries


def _epoch_coo():
    from helpers import zipf_ids
    rng = np.random.default_rng(0)
    row, col = zipf_ids(rng, RN, V), zipf_ids(rng, RN, V)
    col[row == col] = (col[row == col] + 1) % V
    return dict(row=row, col=col, w=rng.uniform(0.1, 1.0, RN).astype(np.float32), y=rng.normal(size=RN).astype(np.float32))


def _epochs_worker(rank, port, out_dir, optimizer):
    _enter(rank, port)
    import glove_ref as ref
    from oracle_backend import OracleTables
    from sharded_oracle_backend import ShardedOracleBackend
    from trainer.data_utils import NonzeroStream
    from trainer.owner_map import balanced_relabel, id_histogram, inverse
    from trainer.stepper import ReshufflingRunner, ShardedStepper, owned_rows
    coo = _epoch_coo()
    perm = balanced_relabel(id_histogram(coo["row"], V), WORLD)
    inv = inverse(perm)
    full = ref.Tables(V, D, optimizer, dtype=np.float64, seed=3)
    own = owned_rows(V, WORLD, rank)
    dt = _f64_tables(optimizer, V_row=own, V_col=own)
    dt.load_whole_state_dict(_whole_state(full), WORLD, rank, relabel=perm)
    shard = _oracle_shard(full, dt)
    tables = OracleTables(shard)
    backend = ShardedOracleBackend()
    stream = NonzeroStream(coo, RB, V, backend, "cpu", rank=rank, world=WORLD, seed=11, static_plans=False, route=dist,
                           cols_by_owner=WORLD, relabel=perm)
    seen = []

    class Recording(ShardedStepper):          # the batches in the order the epochs prepare them = the order they are stepped
        def add_batch(self, row, col, w, y, chunk_cap=0):
            seen.append(tuple(np.asarray(a).copy() for a in (row, col, w, y)))
            return super().add_batch(row, col, w, y, chunk_cap)

    stepper = Recording(backend, tables, _hyper(optimizer), RB, WORLD, rank, dist)
    runner = ReshufflingRunner(None, stream, tables, stepper.hyper, chunk_cap=8, burst=7, stepper=stepper)
    done = 0
    while done < RSTEPS:
        done += runner.run(min(3, RSTEPS - done))
    per = stream.col_per
    out = {"bpe": np.asarray(runner.nb), "nnz": np.asarray(stream.nnz)}
    for s, (r, c, w, y) in enumerate(seen[:RSTEPS]):
        # renamed ids: row u of this rank's shard is u * world + rank, owner-major col id c is (c % per) * world + c // per;
        # the token behind a renamed id p is inv[p]
        out.update({"b%d_row" % s: inv[r.astype(np.int64) * WORLD + rank], "b%d_col" % s: inv[(c % per) * WORLD + c // per],
                    "b%d_w" % s: w, "b%d_y" % s: y})
    np.savez(os.path.join(out_dir, "re%d.npz" % rank), **out)
    _save_gathered(dt, shard, perm, os.path.join(out_dir, "gathered.npz"), rank)
    dist.destroy_process_group()


@pytest.mark.parametrize("optimizer", ["Adagrad", "Adam"])
def test_reshuffled_epochs_with_both_tables_sharded_and_balanced_equal_the_oracle(tmp_path, optimizer):
    """ShardedStepper under the reshuffling runner on a renamed, owner-major stream: 24 steps over four epoch boundaries equal
    the oracle stepping on the ranks' joint per-step batches in original ids; every epoch of a rank visits each of its pairs at
    most once."""
    import glove_ref as ref
    mp.spawn(_epochs_worker, args=(free_port(), str(tmp_path), optimizer), nprocs=WORLD, join=True)
    ranks = [dict(np.load(tmp_path / ("re%d.npz" % r))) for r in range(WORLD)]
    assert sum(int(rk["nnz"]) for rk in ranks) == RN and all(int(rk["bpe"]) * 4 < RSTEPS for rk in ranks)
    t = ref.Tables(V, D, optimizer, dtype=np.float64, seed=3)
    hp = ref.Hyper(learning_rate=0.05)
    coo = _epoch_coo()
    pairs = set(zip(coo["row"].tolist(), coo["col"].tolist(), coo["w"].tolist()))
    for s in range(RSTEPS):
        for rk in ranks:                    # the recorded batches are pairs of the file, in original ids
            assert set(zip(rk["b%d_row" % s].tolist(), rk["b%d_col" % s].tolist(), rk["b%d_w" % s].tolist())) <= pairs
        ref.train_step(t, *[np.concatenate([rk["b%d_%s" % (s, k)] for rk in ranks]) for k in ("row", "col", "w", "y")], hp)
    for rk in ranks:
        bpe = int(rk["bpe"])
        for e in range(RSTEPS // bpe):
            w = np.concatenate([rk["b%d_w" % s] for s in range(e * bpe, (e + 1) * bpe)])
            assert len(w) == bpe * RB and len(np.unique(w)) == len(w)          # (the weights are distinct draws)
    _assert_equals_oracle(np.load(tmp_path / "gathered.npz"), t, RSTEPS)


# ---- 8. checkpoints
def _trained_looking(optimizer, seed):
    """Whole-model DeviceTables (float32, CPU) with non-trivial slots, scalars and global_step."""
    from trainer.hip_api import DeviceTables
    t = DeviceTables(V, D, optimizer, device="cpu", seed=seed)
    gen = torch.Generator().manual_seed(seed)
    for slots in (t.s1, t.s2):
        for x in slots.values():
            x.copy_(torch.rand(x.shape, generator=gen))
    t.scalars.copy_(torch.rand(8, generator=gen))
    t.step.fill_(17)
    return t


def _checkpoint_worker(rank, port, out_dir, both):
    _enter(rank, port)
    from trainer.hip_api import DeviceTables
    from trainer.stepper import owned_rows
    from trainer.train_utils import CheckpointManager
    _, perm = _map_of(_batches())
    own = owned_rows(V, WORLD, rank)
    new = lambda: DeviceTables(V, D, "Adam", device="cpu", seed=100 + rank, V_row=own, V_col=own if both else None)
    saving = new()
    saving.load_whole_state_dict(_trained_looking("Adam", 5).state_dict(), WORLD, rank, relabel=perm)
    saving.R.add_(0.25 * (rank + 1))                         # what a run does: every rank moves its own rows
    saving.s2["br"].mul_(rank + 2.0)
    if both:
        saving.C.sub_(0.5 * (rank + 1))
    view = saving.gathered_state_dict(dist, WORLD, relabel=perm)
    if rank == 0:
        CheckpointManager(out_dir).save(saving, state=view)
    dist.barrier()
    # (b) a modulo run of two ranks takes its rows of the same file; its own gathered view is the saving run's
    modulo = new()
    assert CheckpointManager(out_dir).restore(modulo, shard=(WORLD, rank))
    again = modulo.gathered_state_dict(dist, WORLD)
    # ... and a balanced run resumes to exactly the shard that saved
    resumed = new()
    assert CheckpointManager(out_dir).restore(resumed, shard=(WORLD, rank), relabel=perm)
    for k, v in saving.state_dict().items():
        assert torch.equal(resumed.state_dict()[k], v) if torch.is_tensor(v) else resumed.state_dict()[k] == v, k
    if rank == 0:
        torch.save({"view": view, "again": again}, os.path.join(out_dir, "views.pt"))
    dist.destroy_process_group()


def _assert_same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("both", [False, True])
def test_a_balanced_runs_checkpoint_is_any_runs_checkpoint(tmp_path, both):
    """Saved by a balanced 2-rank run (row-sharded; both tables sharded): restores into an unsharded one-rank run and into a
    modulo 2-rank run, every table and slot bit-equal to the saving run's vocabulary-order view; the file has the keys, shapes
    and dtypes of an unsharded run's checkpoint and nothing about the map."""
    from trainer.hip_api import DeviceTables
    from trainer.train_utils import CheckpointManager
    mp.spawn(_checkpoint_worker, args=(free_port(), str(tmp_path), both), nprocs=WORLD, join=True)
    views = torch.load(tmp_path / "views.pt", weights_only=False)
    _assert_same_state(views["view"], views["again"])
    # the view is the model: token u in row u — the trained-looking whole model with each rank's moves on the rows it owns
    _, perm = _map_of(_batches())
    want = _trained_looking("Adam", 5).state_dict()
    owner = torch.from_numpy(perm % WORLD)
    want["R"] = want["R"] + (0.25 * (owner + 1)).float()[:, None]
    want["slot2_br"] = want["slot2_br"] * (owner + 2.0).float()
    if both:
        want["C"] = want["C"] - (0.5 * (owner + 1)).float()[:, None]
    _assert_same_state(views["view"], want)
    # (a) an unsharded run restores it like its own, and writes the same file
    alone = DeviceTables(V, D, "Adam", device="cpu", seed=1)
    assert CheckpointManager(str(tmp_path)).restore(alone)
    _assert_same_state(alone.state_dict(), views["view"])
    blob = torch.load(tmp_path / "model.ckpt-17.pt", weights_only=False)
    assert sorted(blob) == ["extra", "tables"]
    unsharded = tmp_path / "unsharded"
    CheckpointManager(str(unsharded)).save(alone)
    _assert_same_state(torch.load(unsharded / "model.ckpt-17.pt", weights_only=False)["tables"], blob["tables"])


def test_an_id_map_without_a_shard_is_refused(tmp_path):
    from trainer.hip_api import DeviceTables
    from trainer.train_utils import CheckpointManager
    t = DeviceTables(V, D, "Adagrad", device="cpu", seed=0)
    CheckpointManager(str(tmp_path)).save(t)
    with pytest.raises(ValueError, match="sharded run"):
        CheckpointManager(str(tmp_path)).restore(t, relabel=np.arange(V))
    with pytest.raises(ValueError, match="relabel names"):
        t.load_whole_state_dict(t.state_dict(), 1, 0, relabel=np.arange(V - 1))


# ---- 9. the command line
def test_shard_balance_on_the_command_line(tmp_path):
    from trainer.config_utils import parse_args
    vocab = GOLDEN / "text8_cov90_ctx5_vocab.txt"
    base = ["--disable-datetime-path", "--vocab-txt", str(vocab), "--train-csv", "x.csv"]
    params = parse_args(base + ["--job-dir", str(tmp_path / "a"), "--row-sharded", "--shard-balance", "frequency"])
    assert params["shard_balance"] == "frequency" and params["row_sharded"]
    assert json.loads((tmp_path / "a" / "params.json").read_text())["shard_balance"] == "frequency"
    params = parse_args(base + ["--job-dir", str(tmp_path / "b"), "--row-sharded", "--shard-cols", "--shard-balance", "frequency"])
    assert params["shard_balance"] == "frequency" and params["shard_cols"]
    # alone it is refused, before a job directory is made — the kind of error --shard-cols alone raises
    with pytest.raises(ValueError, match="--shard-balance frequency goes with --row-sharded"):
        parse_args(base + ["--job-dir", str(tmp_path / "c"), "--shard-balance", "frequency"])
    assert not (tmp_path / "c").exists()
    with pytest.raises(ValueError, match="--shard-balance must be one of"):
        parse_args(base + ["--job-dir", str(tmp_path / "d"), "--row-sharded", "--shard-balance", "random"])
    # the defaults are what they were
    plain = parse_args(base + ["--job-dir", str(tmp_path / "e")])
    assert plain["shard_balance"] == "modulo" and not plain["row_sharded"] and not plain["shard_cols"]
    assert json.loads((tmp_path / "e" / "params.json").read_text())["shard_balance"] == "modulo"
    sharded = parse_args(base + ["--job-dir", str(tmp_path / "f"), "--row-sharded"])
    assert sharded["shard_balance"] == "modulo"
