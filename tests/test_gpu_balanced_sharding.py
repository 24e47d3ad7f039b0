"""--shard-balance frequency on the GPU: the sharded steppers on the HIP backend over a stream whose ids were renamed by
trainer.owner_map, every collective through RCCL with one rank, against the float64 oracle stepping on ORIGINAL ids; PREDICT
on the vocabulary-order view; and the CLI with two ranks on the one GPU.

The one-rank RCCL case runs in a process of its own (this file, run as a script): a second RCCL process group inside the pytest
process, behind the one another test made and destroyed, hung (tests/rccl_graph_case.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
for _p in (HERE.parent, HERE.parent / "oracle", HERE):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))
import glove_ref as ref  # noqa: E402
from helpers import SLOTS, free_port, make_batch, opt_tables_from_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = HERE / "golden"
# tests/test_gpu_sharded_optimizers.py's tolerances of a sharded HIP run against the float64 oracle
RTOL, ATOL, ATOL_V, LOSS_RTOL = 2e-5, 2e-6, 1e-9, 1e-5
HIP_LOSS_RTOL = 2e-5                    # ... and of two HIP runs' losses against each other
V, D, B, NB, STEPS = 700, 64, 1500, 3, 7          # three batches per epoch: seven steps cross two epoch boundaries


def _coo():
    return dict(zip(("row", "col", "w", "y"), make_batch(7, NB * B + 77, V)))


def _hyper(optimizer):
    return dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.05 if optimizer == "Adagrad" else 0.01, optimizer=optimizer)


def _run(hip, dist, optimizer, form, epochs, perm):
    """STEPS steps of one sharded form on the HIP backend over NonzeroStream(relabel=perm), the tables cut through the map.
    Returns (tables, stepper, per-step losses, the batches stepped on — in the stream's ids)."""
    from trainer.data_utils import NonzeroStream
    from trainer.hip_api import DeviceTables
    from trainer.stepper import HipBackend, ReshufflingRunner, RowShardedStepper, ShardedStepper
    t = ref.Tables(V, D, optimizer, dtype=np.float32, seed=5).astype(np.float64)
    tabs = DeviceTables(V, D, optimizer, device="cuda:0", seed=0)
    tabs.load_whole_state_dict(opt_tables_from_oracle(t, DeviceTables).state_dict(), 1, 0, relabel=perm)
    backend = HipBackend("cuda:0")
    backend.hip, backend.row_floats = hip, tabs.d
    kw = _hyper(optimizer)
    if form == "both":
        st = ShardedStepper(backend, tabs, kw, B, 1, 0, dist, collectives=True, exercise_exchange=True)
    else:
        st = RowShardedStepper(backend, tabs, kw, B, 1, dist, exchange="rows", collectives=True)
    dealt = epochs == "dealt"
    stream = NonzeroStream(_coo(), B, V, backend, "cuda:0", seed=3, static_plans=not dealt,
                           cols_by_owner=1 if form == "both" and dealt else 0, relabel=perm)
    assert stream.batches_per_epoch == NB
    losses, batches = [], []

    def record(b):
        torch.cuda.synchronize()
        losses.append(float(st.loss_out[0]))
        batches.append(tuple(a.cpu().numpy().copy() for a in stream.batch(b)))
    if dealt:
        assert stream.masters is not None
        if form != "both":
            st.prepare(batch_size=B)
        runner = ReshufflingRunner(hip, stream, tabs, st.hyper, burst=4, segment=2, stepper=st, graphs=False)
        for _ in range(STEPS):
            assert runner.run(1) == 1
            record(runner.position - 1)
        keep = runner
    else:
        if form == "both":
            items = [st.add_batch(*(a.contiguous() for a in stream.batch(b))) for b in range(NB)]
        else:
            st.prepare(stream.plans)
            items = stream.plans
        for _ in range(STEPS):
            stream.next_plan()
            st.step(items[stream.last_batch])
            record(stream.last_batch)
        keep = None
    return tabs, st, losses, batches, keep


def _assert_state_equals_oracle(state, scalars, t, what):
    for n in ("R", "C", "br", "bc"):
        np.testing.assert_allclose(state[n].numpy(), getattr(t, n), rtol=RTOL, atol=ATOL, err_msg="%s %s" % (what, n))
        for k, pre in enumerate(SLOTS[t.optimizer]):
            np.testing.assert_allclose(state["slot%d_%s" % (k + 1, n)].numpy(), getattr(t, pre + n), rtol=RTOL,
                                       atol=ATOL_V if pre == "V_" else ATOL, err_msg="%s %s%s" % (what, pre, n))
    sc = scalars.cpu().numpy().astype(np.float64)
    want = [t.g] + [getattr(t, pre + "g") for pre in SLOTS[t.optimizer]]
    np.testing.assert_allclose(sc[:len(want)], want, rtol=RTOL, atol=ATOL_V, err_msg=what + " scalars")
    assert int(state["global_step"]) == t.step == STEPS, what


def case(out_dir):
    """Run as a script: one rank, RCCL.  Every (optimizer, form, epochs): the relabelled HIP run, gathered to vocabulary order
    through gathered_state_dict(relabel=), against the float64 oracle stepping on the same batches in original ids — tables,
    slots, scalars and the loss of every step.  Static epochs cut the same pairs into the same batches with and without the
    map (the stream's permutation does not look at ids), so there the loss curve of the unrelabelled HIP run is compared step
    by step as well; a dealt epoch seats the pairs by their place in the id-sorted master orders, so renaming ids changes
    which pairs share a batch: there each HIP run is held to the oracle on its own batches instead.  Relabelling changes the
    order of partners inside an id's run: no bit-identity between the two HIP runs is asserted anywhere."""
    import faulthandler
    import torch.distributed as dist
    from trainer.hip_api import GloveHip
    from trainer.owner_map import balanced_relabel, id_histogram, inverse
    faulthandler.dump_traceback_later(240, exit=True)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ["CASE_PORT"], RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", device_id=torch.device("cuda:0"))
    alive = []
    try:
        hip = GloveHip("cuda:0")
        counts = id_histogram(_coo()["row"], V)
        perm = balanced_relabel(counts, 1)
        inv = inverse(perm)
        np.testing.assert_array_equal(inv, np.argsort(-counts, kind="stable"))      # alone in the world: count-descending order
        assert np.count_nonzero(perm != np.arange(V)) > V // 2                      # ... a non-trivial permutation
        last = None
        for optimizer in ("Adagrad", "Adam"):
            hp = ref.Hyper(learning_rate=_hyper(optimizer)["learning_rate"])
            for form in ("rows", "both"):
                for epochs in ("static", "dealt"):
                    what = "%s, %s, %s epochs" % (optimizer, "row-sharded" if form == "rows" else "both tables sharded", epochs)
                    curves = {}
                    for name, p in (("relabelled", perm), ("plain", None)):
                        tabs, st, losses, batches, keep = _run(hip, dist, optimizer, form, epochs, p)
                        alive.append(keep)
                        back = inv if p is not None else np.arange(V)
                        t = ref.Tables(V, D, optimizer, dtype=np.float32, seed=5).astype(np.float64)
                        want = [ref.train_step(t, back[r], back[c], w, y, hp)[0] for r, c, w, y in batches]
                        curves[name] = losses
                        err = max(abs(a - b) / abs(b) for a, b in zip(losses, want))
                        print("%s, %s ids: max relative loss error against the oracle %.2e" % (what, name, err), flush=True)
                        np.testing.assert_allclose(losses, want, rtol=LOSS_RTOL, err_msg="%s %s loss" % (what, name))
                        state = tabs.gathered_state_dict(dist, 1, relabel=p)
                        _assert_state_equals_oracle(state, tabs.scalars, t, "%s %s" % (what, name))
                        if p is not None:
                            # the tables themselves are NOT in vocabulary order: the view is what the map gives back
                            assert not torch.equal(tabs.embeddings("R").cpu(), state["R"])
                            last = (tabs, state, optimizer)
                    if epochs == "static":
                        err = max(abs(a - b) / abs(b) for a, b in zip(curves["relabelled"], curves["plain"]))
                        print("%s: max relative loss difference between the two HIP runs %.2e" % (what, err), flush=True)
                        np.testing.assert_allclose(curves["relabelled"], curves["plain"], rtol=HIP_LOSS_RTOL, err_msg=what)
        _predict_case(hip, dist, perm, out_dir, *last)
    finally:
        import gc
        from trainer.stepper import ReshufflingRunner, RowShardedStepper, ShardedStepper
        for obj in gc.get_objects():
            if isinstance(obj, (RowShardedStepper, ShardedStepper, ReshufflingRunner)):
                obj.release_graphs()
        gc.collect()
        dist.destroy_process_group()
    print("balanced sharding case ok", flush=True)


def _predict_case(hip, dist, perm, out_dir, tabs, state, optimizer):
    """PREDICT after such a run: the Estimator's vocabulary-order view of the sharded, renamed tables gives the top-k token
    strings of the same checkpoint restored unsharded."""
    from types import SimpleNamespace
    from trainer.estimator import Estimator
    from trainer.hip_api import DeviceTables
    from trainer.model_utils import get_predictions
    from trainer.stepper import HipBackend
    from trainer.train_utils import CheckpointManager
    backend = HipBackend("cuda:0")
    backend.hip = hip
    CheckpointManager(out_dir).save(tabs, state=state)
    plain = DeviceTables(V, D, optimizer, device="cuda:0", seed=1)
    assert CheckpointManager(out_dir).restore(plain)
    sharded_run = SimpleNamespace(row_sharded=True, model=SimpleNamespace(tables=tabs), dist=dist, world=1,
                                  relabel=torch.from_numpy(perm))
    view = Estimator._vocabulary_order_model(sharded_run)
    tokens = ["tok%d" % i for i in range(V)]
    ids = torch.arange(0, V, 7, dtype=torch.int32)
    got = get_predictions(backend, view, ids, tokens, 10)
    want = get_predictions(backend, SimpleNamespace(tables=plain), ids, tokens, 10)
    assert got["input_string"] == want["input_string"] == ["tok%d" % i for i in ids.tolist()]
    assert got["top_k_string"] == want["top_k_string"]
    assert all(row[0] == tok for row, tok in zip(got["top_k_string"], got["input_string"]))       # a token is its own nearest
    assert torch.equal(got["input_embedding"], want["input_embedding"])
    assert torch.equal(got["top_k_similarity"], want["top_k_similarity"])
    # ... and not those of the tables read as they lie (renamed order)
    lying = get_predictions(backend, SimpleNamespace(tables=tabs), ids, tokens, 10)
    assert lying["top_k_string"] != want["top_k_string"]


def test_relabelled_sharded_steps_and_predict_on_the_hip_backend(hip, tmp_path):
    """ShardedStepper and RowShardedStepper over NonzeroStream(relabel=balanced_relabel(counts, 1)), static and dealt epochs,
    Adagrad and Adam, through RCCL with one rank == the float64 oracle on original ids; PREDICT on the vocabulary-order view
    (`case` and `_predict_case` above say what is compared)."""
    env = dict(os.environ, CASE_PORT=str(free_port()))
    proc = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(tmp_path)], capture_output=True, text=True,
                          timeout=280, env=env)
    print(proc.stdout[-6000:])
    assert proc.returncode == 0 and "balanced sharding case ok" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-5000:]


def _two_rank_balanced_trainer(rank, port, argv, out_dir):
    """One rank of `python -m trainer.estimator --shard-balance frequency` (as tests/test_gpu_trainer.py's _two_rank_trainer:
    both ranks on the one GPU, gloo transport), then PREDICT from the sharded run (collective) on both ranks."""
    import torch.distributed as dist
    for p in (HERE.parent, HERE):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    from trainer import estimator
    from trainer.config_utils import parse_args
    from trainer.stepper import HipBackend
    dist.init_process_group("gloo", rank=rank, world_size=2)
    box = [parse_args(argv) if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    params = box[0]
    est = estimator.Estimator(params, backend=HipBackend("cuda:0"), dist=dist, device="cuda:0")
    est.train(params["train_steps"])
    predictions = [(p["input_string"], p["top_k_string"]) for p in est.predict()]
    t = est.model.tables
    torch.save({"relabel": est.relabel, "imbalance": est.stream().load_imbalance, "rows": t.V_row, "step": t.global_step,
                "predictions": predictions}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


@pytest.mark.parametrize("extra", [["--row-sharded"], ["--row-sharded", "--shard-cols"]], ids=["rows", "both"])
def test_two_rank_cli_with_frequency_balanced_ownership_on_one_gpu(hip, tmp_path, extra):
    """`--shard-balance frequency` end to end, two ranks on the one GPU: the ranks' shares of the nonzeros are closer than
    id % ranks leaves them, training lowers the loss over the whole file below the initial model's, the checkpoint is in
    vocabulary order (one unsharded process evaluates it to the loss the two ranks computed, and predicts what they predict), a
    modulo run of two ranks takes exactly its rows out of it and trains on, and so does one process.
    (Progress is judged by the eval pass over all 620 nonzeros against the seeded initial model, not by two lines of the
    training log: a logged loss is that of one batch of 96 pairs, and its noise exceeds what ten steps gain.)"""
    import torch.multiprocessing as mp
    from test_gpu_trainer import _two_rank_trainer
    from trainer import estimator
    from trainer.owner_map import balanced_relabel, id_histogram, imbalance, shard_loads
    csv, vocab = GOLDEN / "text8_cov90_ctx5_interaction.csv", GOLDEN / "text8_cov90_ctx5_vocab.txt"
    n_tokens = len(vocab.read_text().split("\n"))
    job = tmp_path / "job"
    base = ["--train-csv", str(csv), "--vocab-txt", str(vocab), "--disable-datetime-path", "--embedding-size", "24",
            "--optimizer", "Adam", "--batch-size", "48", "--job-dir", str(job), "--seed", "9"]
    argv = base + ["--train-steps", "90", "--log-every", "30"] + extra
    mp.spawn(_two_rank_balanced_trainer, args=(free_port(), argv + ["--shard-balance", "frequency"], str(tmp_path)), nprocs=2,
             join=True)
    a, b = (torch.load(tmp_path / ("rank%d.pt" % r), weights_only=False) for r in range(2))
    assert a["step"] == b["step"] == 90 and a["rows"] + b["rows"] == n_tokens
    # every rank computed the same map, the one the data gives, and the stream measured the ratio the map promises
    params = json.loads((job / "params.json").read_text())
    assert params["shard_balance"] == "frequency"
    coo = estimator.load_interaction_csv(str(csv), params["vocab_txt"], *params["input_fn_args"]["select_columns"])
    counts = id_histogram(coo["row"], n_tokens)
    perm = balanced_relabel(counts, 2)
    assert torch.equal(a["relabel"], b["relabel"]) and np.array_equal(a["relabel"].numpy(), perm)
    balanced, modulo = imbalance(shard_loads(counts, perm, 2)), imbalance(shard_loads(counts, None, 2))
    assert a["imbalance"] == b["imbalance"] == balanced < modulo
    log = [json.loads(l) for l in (job / "train_log.jsonl").read_text().splitlines()]
    assert [r["global_step"] for r in log] == [30, 60, 90] and all(np.isfinite(r["loss"]) for r in log), log
    ev = [json.loads(l) for l in (job / "eval" / "eval_log.jsonl").read_text().splitlines()]
    assert ev[-1]["global_step"] == 90
    # the model the ranks started from (seeded; rank 0's init), evaluated by one process: training went down from there
    (tmp_path / "initial").mkdir()
    untrained = dict(params, job_dir=str(tmp_path / "initial"), row_sharded=False, shard_cols=False, shard_balance="modulo")
    initial_loss = estimator.Estimator(untrained).evaluate()["average_loss"]
    print("average_loss over the file: initial %.6f, after 90 steps %.6f" % (initial_loss, ev[-1]["average_loss"]))
    assert ev[-1]["average_loss"] < initial_loss
    blob = torch.load(job / "model.ckpt-90.pt", weights_only=False)["tables"]
    assert blob["V_row"] == n_tokens and all(blob[k].shape == (n_tokens, 24) for k in ("R", "C", "slot1_R", "slot2_C"))
    assert not any("relabel" in k or "perm" in k for k in blob)
    # vocabulary order: one process on plain tables evaluates the file to the loss the two ranks computed ...
    params.update(row_sharded=False, shard_cols=False, shard_balance="modulo")
    alone = estimator.Estimator(params)
    np.testing.assert_allclose(alone.evaluate()["average_loss"], ev[-1]["average_loss"], rtol=1e-5)
    # ... and predicts, token by token, what the sharded run predicted
    want = [(p["input_string"], p["top_k_string"]) for p in alone.predict()]
    assert a["predictions"] == b["predictions"] == want
    # a modulo run of two ranks resumes from it: asked for no further step it holds exactly its rows of the file, id % 2 ...
    more = base + ["--log-every", "10"]
    both = "--shard-cols" in extra
    (tmp_path / "restored").mkdir()
    mp.spawn(_two_rank_trainer, args=(free_port(), more + ["--train-steps", "90"] + extra, str(tmp_path / "restored")), nprocs=2,
             join=True)
    for r in range(2):
        got = torch.load(tmp_path / "restored" / ("rank%d.pt" % r))
        assert got["step"] == 90
        assert torch.equal(got["R"], blob["R"][r::2]) and torch.equal(got["br"], blob["br"][r::2])
        assert torch.equal(got["C"], blob["C"][r::2] if both else blob["C"])
        assert torch.equal(got["bc"], blob["bc"][r::2] if both else blob["bc"])
    # ... and trains on from there, then a single process does
    (tmp_path / "resumed").mkdir()
    mp.spawn(_two_rank_trainer, args=(free_port(), more + ["--train-steps", "100"] + extra, str(tmp_path / "resumed")), nprocs=2,
             join=True)
    assert torch.load(tmp_path / "resumed" / "rank0.pt")["step"] == 100 and (job / "model.ckpt-100.pt").exists()
    log = [json.loads(l) for l in (job / "train_log.jsonl").read_text().splitlines()]
    assert log[-1]["global_step"] == 100 and np.isfinite(log[-1]["loss"])
    ev = [json.loads(l) for l in (job / "eval" / "eval_log.jsonl").read_text().splitlines()]
    assert ev[-1]["global_step"] == 100 and ev[-1]["average_loss"] < initial_loss
    estimator.main(more + ["--train-steps", "110"])
    assert (job / "model.ckpt-110.pt").exists()


if __name__ == "__main__":
    case(sys.argv[1])
