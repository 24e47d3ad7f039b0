"""The sharded multi-GPU forms under every Keras optimizer, on the GPU: the touched-rows apply of the dense-decay optimizers
(Adam, RMSprop, Nadam) restricted to one side against the float64 oracle, the sharded steppers alone in the world against the
plain single-GPU step, every form through RCCL with one rank, and the CLI with two ranks on the one GPU.
(The same apply at every row shape, on lists of several ranks and on lists longer than one grid sweep: tests/test_gpu_exchange_row_shapes.py.)"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent / "oracle"))
import glove_ref as ref  # noqa: E402
from helpers import assert_opt_tables_close, free_port, make_batch, opt_tables_from_oracle, to_dev  # noqa: E402
from sharded_oracle_backend import restricted_update  # noqa: E402

pytestmark = pytest.mark.gpu
OPTIMIZERS = ("Adagrad", "SGD", "RMSprop", "Adamax", "Adam", "Adadelta", "Ftrl", "Nadam")
ROWS_ONLY = ("SGD", "Adamax", "Adadelta", "Ftrl", "Nadam")
GOLDEN = HERE / "golden"


def _seeded_tables(V, d, optimizer, seed):
    """Oracle tables whose slots hold non-trivial state (the sweep's decay must show), at global_step 3."""
    rng = np.random.default_rng(seed)
    t = ref.Tables(V, d, optimizer, dtype=np.float32, seed=seed).astype(np.float64)
    for n in ("R", "C", "br", "bc"):
        shape = getattr(t, n).shape
        if optimizer in ("Adam", "Nadam"):
            setattr(t, "M_" + n, rng.normal(0, 1e-3, shape).astype(np.float32).astype(np.float64))
            setattr(t, "V_" + n, rng.uniform(1e-7, 1e-5, shape).astype(np.float32).astype(np.float64))
        else:
            setattr(t, "A_" + n, rng.uniform(1e-4, 1e-3, shape).astype(np.float32).astype(np.float64))
    t.step = 3
    if optimizer == "Nadam":
        t.m_cache = np.float64(np.float32(0.61))
    return t


def _lists(rng, V, d, stride, sides, n_lists=3):
    """n_lists bare lists of entries naming their side: ids named by one list only, ids named by several, the last list empty."""
    out = []
    shared = {s: rng.choice(V, 40, replace=False) for s in (0, 1)}
    for k in range(n_lists):
        rows = []
        for side, bit in ((0, 1), (1, 2)):
            if not sides & bit or k == n_lists - 1:
                continue
            own = rng.choice(V, 200, replace=False)
            ids = np.unique(np.concatenate([own, shared[side]]))
            e = np.zeros((len(ids), stride + 4), np.float32)
            e[:, :d] = rng.normal(0, 0.01, (len(ids), d))
            e[:, stride] = rng.normal(0, 0.01, len(ids))
            e.view(np.int32)[:, stride + 1] = ids
            e.view(np.int32)[:, stride + 2] = side
            rows.append(e)
        out.append(np.concatenate(rows) if rows else np.zeros((0, stride + 4), np.float32))
    return out


def _oracle_sums(t, lists, d, stride):
    gr = dict(G_R=np.zeros_like(t.R), G_C=np.zeros_like(t.C), G_br=np.zeros_like(t.br), G_bc=np.zeros_like(t.bc),
              touched_r=np.zeros(len(t.R), bool), touched_c=np.zeros(len(t.C), bool))
    for e in lists:                                          # in list (rank) order
        for row in e.astype(np.float64):
            i, side = int(np.float32(row[stride + 1]).view(np.int32)), int(np.float32(row[stride + 2]).view(np.int32))
            W, b, tch = ("G_R", "G_br", "touched_r") if side == 0 else ("G_C", "G_bc", "touched_c")
            gr[W][i] += row[:d]
            gr[b][i] += row[stride]
            gr[tch][i] = True
    return gr


APPLY_CASES = [(o, s, V, d) for o in ("Adam", "RMSprop", "Nadam") for s in (1, 2, 3)
               for V, d in ((3000, 64), (2000, 128), (1500, 300))] + [("Adam", 2, 400_000, 64), ("Adam", 3, 400_000, 64)]


@pytest.mark.parametrize("optimizer,sides,V,d", APPLY_CASES)
def test_touched_rows_apply_of_the_dense_decay_optimizers_on_one_side(hip, optimizer, sides, V, d):
    """glove_apply_packed_adagrad_f32 under Adam / RMSprop / Nadam with hyper.sides 1, 2, 3: the listed rows of the selected
    sides take the lists' summed gradients, every other row of them its G = 0 update, the other side stays as it was; the
    scalar work with the col side."""
    from trainer.hip_api import DeviceTables, make_hyper
    rng = np.random.default_rng(V + d + sides)
    t = _seeded_tables(V, d, optimizer, 11)
    dt = opt_tables_from_oracle(t, DeviceTables)
    dt.step.fill_(4)                                         # as this step's row pass leaves it
    stride = dt.d
    lists = _lists(rng, V, d, stride, sides)
    bufs = [torch.from_numpy(e if len(e) else np.zeros((1, stride + 4), np.float32)).cuda() for e in lists]
    packed = [hip.packed_list(b, with_header=False, n=len(e)) for b, e in zip(bufs, lists)]
    G = hip.dense_grad_buffer(dt)
    mark = torch.zeros(dt.V_row + dt.V, dtype=torch.int32, device="cuda:0")
    tail = torch.tensor([0.3, 2.0, 5.0, 1.0], device="cuda:0")
    hp = ref.Hyper(learning_rate=0.01)
    h = make_hyper(learning_rate=hp.learning_rate, batch_size=4096, sides=sides, optimizer=optimizer)
    loss_out = torch.zeros(4, device="cuda:0")
    scalars_before = dt.scalars.clone()
    hip.count_packed(packed, dt, G, mark, 0)
    for k, lst in enumerate(packed):
        hip.combine_packed(lst, k, dt, G, mark, 0)
    hip.apply_packed(packed, dt, h, G, mark, tail if sides & 2 else None, loss_out, 0)
    torch.cuda.synchronize()
    gr = _oracle_sums(t, lists, d, stride)
    gr["sum_e"] = 0.3
    restricted_update(t, gr, hp, sides)
    if not sides & 2:                    # no scalar work: the scalars (global bias, its slots, the momentum cache) untouched
        t.step = 4                       # (global_step as this step's pass left it)
        assert torch.equal(dt.scalars.view(torch.int32), scalars_before.view(torch.int32))
    _assert_tables_close(dt, t, scalar_work=bool(sides & 2))
    assert int(mark.abs().sum()) == 0, "marks left behind"


@pytest.mark.parametrize("optimizer", OPTIMIZERS)
def test_row_side_step_of_every_optimizer(hip, optimizer):
    """glove_rowside_step_f32 behind the col pass: the row table and its slots take the optimizer's update on the batch's row
    gradients (Adam, RMSprop, Nadam: every row of it moves its slots), the col side and the scalars stay for the col apply."""
    from trainer.hip_api import DeviceTables, make_hyper
    B, V, d = 3000, 900, 64
    t = _seeded_tables(V, d, optimizer, 7) if optimizer in ("Adam", "Nadam", "RMSprop") else \
        ref.Tables(V, d, optimizer, dtype=np.float32, seed=7).astype(np.float64)
    dt = opt_tables_from_oracle(t, DeviceTables)
    row, col, w, y = make_batch(5, B, V)
    plan = hip.build_plan(*to_dev(row, col, w, y), V)
    hp = ref.Hyper(learning_rate=0.01, momentum=0.9 if optimizer == "SGD" else 0.0)
    kw = dict(learning_rate=hp.learning_rate, momentum=hp.momentum, batch_size=B, optimizer=optimizer)
    # the scratch: V_row marks (Adam, Nadam), the row half of a dense gradient buffer (RMSprop); NaN-free zeros behind it
    n = hip.grad_layout(dt)["G_C"] if optimizer == "RMSprop" else V
    G = torch.zeros(n, device="cuda:0")
    scalars_before = dt.scalars.clone()
    hip.colpass(plan, dt, make_hyper(sides=2, **kw))
    hip.rowside_step_opt(plan, dt, make_hyper(sides=1, **kw), G if optimizer in ("Adam", "RMSprop", "Nadam") else None)
    torch.cuda.synchronize()
    step = t.step
    gr = ref.gradients(t, row, col, w, y, hp)
    restricted_update(t, gr, hp, 1)
    t.step = step + 1
    # the scalars (global bias, its slots, Nadam's momentum cache) are the col apply's: untouched here
    assert torch.equal(dt.scalars.view(torch.int32), scalars_before.view(torch.int32))
    _assert_tables_close(dt, t, scalar_work=False)
    assert float(G.abs().max()) == 0.0, "scratch left dirty"


def _assert_tables_close(dt, t, scalar_work):
    """assert_opt_tables_close; without the scalar work Nadam's momentum cache is left out of it (the caller asserted that the
    scalars did not move: the slot the comparison reads was never written, it holds what opt_tables_from_oracle put there)."""
    if scalar_work or t.optimizer != "Nadam":
        return assert_opt_tables_close(dt, t)
    import copy
    tc = copy.copy(t)
    tc.optimizer = "Adamax"              # the same two slots (m, v) and no momentum cache in the comparison
    assert_opt_tables_close(dt, tc)


def _tables_state(tabs):
    out = {n: getattr(tabs, n).clone() for n in ("R", "C", "br", "bc")}
    for k, s in (("s1", tabs.s1), ("s2", tabs.s2)):
        for n, x in s.items():
            out[k + n] = x.clone()
    out["scalars"], out["step"] = tabs.scalars.clone(), tabs.global_step
    return out


def test_sharded_steppers_alone_in_the_world_are_the_plain_adam_step(hip):
    """World 1 without the exchange: RowShardedStepper and ShardedStepper run exactly the single-GPU Adam step."""
    from trainer.hip_api import DeviceTables
    from trainer.stepper import HipBackend, RowShardedStepper, ShardedStepper, Stepper
    B, V, d, steps = 6000, 700, 64, 4
    backend = HipBackend("cuda:0")
    t = ref.Tables(V, d, "Adam", dtype=np.float32, seed=4).astype(np.float64)
    kw = dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.01, optimizer="Adam")
    batches = [to_dev(*make_batch(40 + s, B, V)) for s in range(steps)]
    plans = [backend.build_plan(*bt, V, 0) for bt in batches]
    plain_t, row_t, both_t = (opt_tables_from_oracle(t, DeviceTables) for _ in range(3))
    plain = Stepper(backend, plain_t, kw, B)
    row = RowShardedStepper(backend, row_t, kw, B, 1, None)
    both = ShardedStepper(backend, both_t, kw, B, 1, 0, None)
    handles = [both.add_batch(*bt) for bt in batches]
    for s in range(steps):
        plain.step(plans[s])
        row.step(plans[s])
        both.step(handles[s])
    want = _tables_state(plain_t)
    for name, tabs in (("row-sharded", row_t), ("both sharded", both_t)):
        got = _tables_state(tabs)
        for k in want:
            assert (got[k] == want[k]) if k == "step" else torch.equal(got[k], want[k]), (name, k)
    assert want["step"] == steps


def _close(a, b, what, rtol=2e-5, atol=2e-6):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: what + ": " + m)


def test_every_optimizer_on_every_sharded_form_through_rccl_with_one_rank(hip):
    """All eight names x {row-sharded with the dense col exchange, with the lists, both tables sharded}, every collective through
    RCCL on this one GPU (a process group of one rank, `collectives=True`, the fully sharded form's exchange exercised): each
    equals the plain single-GPU step of the optimizer — weights, every slot, the scalars, global_step."""
    import os
    import torch.distributed as dist
    from trainer.hip_api import DeviceTables
    from trainer.stepper import HipBackend, RowShardedStepper, ShardedStepper, Stepper
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", device_id=torch.device("cuda:0"))
    try:
        B, V, d, steps = 6000, 700, 64, 4
        backend = HipBackend("cuda:0")
        batches = [to_dev(*make_batch(60 + s, B, V)) for s in range(steps)]
        plans = [backend.build_plan(*bt, V, 0).compact(hip.lib, d) for bt in batches]
        for opt in OPTIMIZERS:
            t = ref.Tables(V, d, opt, dtype=np.float32, seed=5).astype(np.float64)
            kw = dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.01 if opt != "Adagrad" else 0.05, optimizer=opt)
            if opt == "SGD":
                kw.update(momentum=0.9)
            plain_t = opt_tables_from_oracle(t, DeviceTables)
            plain = Stepper(backend, plain_t, kw, B)
            runs = {}
            for exchange in ("dense", "rows"):
                if exchange == "dense" and opt in ROWS_ONLY:
                    continue
                tabs = opt_tables_from_oracle(t, DeviceTables)
                st = RowShardedStepper(backend, tabs, kw, B, 1, dist, exchange=exchange, collectives=True)
                st.prepare(plans)
                assert st.rows == (exchange == "rows")
                runs["row-sharded, " + exchange] = (tabs, st, plans)
            tabs = opt_tables_from_oracle(t, DeviceTables)
            st = ShardedStepper(backend, tabs, kw, B, 1, 0, dist, collectives=True, exercise_exchange=True)
            runs["both tables sharded"] = (tabs, st, [st.add_batch(*bt) for bt in batches])
            for s in range(steps):
                plain.step(plans[s])
                for tabs, st, items in runs.values():
                    st.step(items[s])
            want = _tables_state(plain_t)
            for name, (tabs, st, _) in runs.items():
                got = _tables_state(tabs)
                for k in want:
                    if k == "step":
                        assert got[k] == want[k] == steps, (opt, name)
                    elif k == "scalars":
                        _close(got[k][:3], want[k][:3], "%s %s scalars" % (opt, name))
                        if opt == "Nadam":
                            _close(got[k][4 + steps % 2], want[k][4 + steps % 2], "%s %s momentum cache" % (opt, name))
                    else:
                        _close(got[k], want[k], "%s %s %s" % (opt, name, k),
                               atol=1e-9 if opt == "Adam" and k.startswith("s2") else 2e-6)
                np.testing.assert_allclose(st.read_loss()["loss"], plain.read_loss()["loss"], rtol=2e-5, err_msg=opt + " " + name)
    finally:
        dist.destroy_process_group()


def test_sharded_adam_steps_replayed_from_hipgraphs(hip):
    """A sharded step under Adam / RMSprop / Nadam captured ONCE as a hipGraph — kernels, the row side's scratch, the owner's
    apply with its own hyper, the RCCL collectives of one rank — and replayed == the eager steps, bit for bit."""
    import os
    import subprocess
    # (in a process of its own: tests/rccl_graph_case.py says why)
    env = dict(os.environ, CASE_PORT=str(free_port()))
    proc = subprocess.run([sys.executable, str(HERE / "sharded_graph_case.py")], capture_output=True, text=True, timeout=280, env=env)
    assert proc.returncode == 0 and "sharded graph case ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


def _two_rank_sharded_adam(rank, port, out_dir, V, d, B, steps):
    """Two ranks on the one GPU over gloo, both tables sharded, Adam."""
    import os
    import torch.distributed as dist
    for p in (HERE.parent, HERE.parent / "oracle", HERE):
        sys.path.insert(0, str(p))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    from trainer.hip_api import DeviceTables
    from trainer.stepper import HipBackend, ShardedStepper, owned_rows, route_by_row_owner
    dist.init_process_group("gloo", rank=rank, world_size=2)
    t = ref.Tables(V, d, "Adam", dtype=np.float32, seed=7).astype(np.float64)
    own = owned_rows(V, 2, rank)
    shard = DeviceTables(V, d, "Adam", device="cuda:0", seed=0, V_row=own, V_col=own)     # m, v: zeros, as the oracle's
    for n in ("R", "C", "br", "bc"):
        getattr(shard, n).copy_(torch.from_numpy(getattr(t, n)[rank::2].astype(np.float32)))
    st = ShardedStepper(HipBackend("cuda:0"), shard, dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.01, optimizer="Adam"), B, 2,
                        rank, dist)
    handles = []
    for k in range(steps):
        row, col, w, y = make_batch(5000 + 10 * k + rank, B, V)
        if k == steps - 1:                # a step whose col ids all belong to rank 0 (even ids): rank 1 serves nothing
            col = (col // 2 * 2) % V
            col[col == row] = (col[col == row] + 2) % V
        row, col, w, y = to_dev(row, col.astype(np.int32), w, y)
        got = route_by_row_owner(dict(row=row, col=col, w=w, y=y), 2, rank, dist)
        handles.append(st.add_batch(got["row"], got["col"], got["w"], got["y"], 16))
    for h in handles:
        st.step(h)
    out = {n: getattr(shard, n).cpu() for n in ("R", "C", "br", "bc")}
    out.update({"M_" + n: shard.s1[n].cpu() for n in shard.s1})
    out.update({"V_" + n: shard.s2[n].cpu() for n in shard.s2})
    out.update(scalars=shard.scalars.cpu(), step=shard.global_step, loss=st.read_loss())
    torch.save(out, os.path.join(out_dir, "shard%d.pt" % rank))
    dist.destroy_process_group()


def test_two_rank_fully_sharded_adam_step_on_one_gpu(hip, tmp_path):
    """Both tables sharded under Adam, two ranks sharing the box's GPU (gloo transport, HIP kernels; the lists of two ranks,
    a step in which one rank serves nothing): the float64 oracle stepping on the union of the ranks' batches — weights, m,
    v, the global bias with its moments, global_step."""
    import torch.multiprocessing as mp
    V, d, B, steps = 2001, 64, 3000, 4
    mp.spawn(_two_rank_sharded_adam, args=(free_port(), str(tmp_path), V, d, B, steps), nprocs=2, join=True)
    t = ref.Tables(V, d, "Adam", dtype=np.float32, seed=7).astype(np.float64)
    hp = ref.Hyper(learning_rate=0.01)
    for k in range(steps):
        parts = [list(make_batch(5000 + 10 * k + r, B, V)) for r in range(2)]
        if k == steps - 1:
            for p_ in parts:
                p_[1] = ((p_[1] // 2 * 2) % V).astype(np.int32)
                p_[1][p_[1] == p_[0]] = (p_[1][p_[1] == p_[0]] + 2) % V
        loss, _, _ = ref.train_step(t, *[np.concatenate(x) for x in zip(*parts)], hp)
    for r in range(2):
        s_ = torch.load(tmp_path / ("shard%d.pt" % r))
        for n in ("R", "C", "br", "bc"):
            for pre in ("", "M_", "V_"):
                np.testing.assert_allclose(s_[pre + n].numpy(), getattr(t, pre + n)[r::2], rtol=2e-5,
                                           atol=1e-9 if pre == "V_" else 2e-6, err_msg=pre + n)
        sc = s_["scalars"].numpy().astype(np.float64)
        np.testing.assert_allclose(sc[:3], [t.g, t.M_g, t.V_g], rtol=2e-5, atol=1e-9)
        assert s_["step"] == steps
        np.testing.assert_allclose(s_["loss"]["loss"], loss, rtol=1e-5)


def test_two_rank_adam_cli_row_sharded_and_both_sharded_on_one_gpu(hip, tmp_path):
    """`--optimizer Adam --row-sharded [--shard-cols]`, the other flags at their defaults, two ranks on the one GPU: the eval
    training loss falls, the checkpoint holds the whole model with the whole m and v, the same level as an unsharded run with the same
    seed, and one unsharded process resumes training from it."""
    import torch.multiprocessing as mp
    from test_gpu_trainer import _two_rank_trainer
    from trainer import estimator
    csv, vocab = GOLDEN / "text8_cov90_ctx5_interaction.csv", GOLDEN / "text8_cov90_ctx5_vocab.txt"
    V = len(vocab.read_text().split("\n"))
    base = ["--train-csv", str(csv), "--vocab-txt", str(vocab), "--disable-datetime-path", "--embedding-size", "24",
            "--optimizer", "Adam", "--batch-size", "48", "--train-steps", "90", "--log-every", "30", "--seed", "9"]
    plain = tmp_path / "plain"
    estimator.main(base + ["--job-dir", str(plain / "job")])
    ref_loss = json.loads((plain / "job" / "eval" / "eval_log.jsonl").read_text().splitlines()[-1])["average_loss"]
    for name, extra in (("rows", ["--row-sharded"]), ("both", ["--row-sharded", "--shard-cols"])):
        out = tmp_path / name
        out.mkdir()
        job = out / "job"
        argv = base + ["--job-dir", str(job)] + extra
        mp.spawn(_two_rank_trainer, args=(free_port(), argv, str(out)), nprocs=2, join=True)
        a, b = (torch.load(out / ("rank%d.pt" % r)) for r in range(2))
        assert a["R"].shape[0] + b["R"].shape[0] == V and a["step"] == b["step"] == 90 and a["g"] == b["g"]
        log = [json.loads(l) for l in (job / "train_log.jsonl").read_text().splitlines()]
        assert [r["global_step"] for r in log] == [30, 60, 90] and log[-1]["loss"] < log[0]["loss"], (name, log)
        ev = [json.loads(l) for l in (job / "eval" / "eval_log.jsonl").read_text().splitlines()]
        assert ev[-1]["global_step"] == 90, (name, ev)
        blob = torch.load(job / "model.ckpt-90.pt", weights_only=False)["tables"]
        for k in ("R", "C", "slot1_R", "slot2_R", "slot1_C", "slot2_C"):
            assert blob[k].shape == (V, 24), (name, k)
        # the whole-model checkpoint IS the model the ranks trained: one process on plain tables evaluates it to the loss the two
        # ranks computed (as tests/test_gpu_trainer.py:770); the training level is the unsharded run's (its batches differ: a
        # data-parallel rank takes a slice of the stream, a sharded one the pairs of its rows; as test_gpu_trainer.py:764)
        params = json.loads((job / "params.json").read_text())
        params.update(row_sharded=False, shard_cols=False)
        np.testing.assert_allclose(estimator.Estimator(params).evaluate()["average_loss"], ev[-1]["average_loss"], rtol=1e-5,
                                   err_msg=name)
        np.testing.assert_allclose(ev[-1]["average_loss"], ref_loss, rtol=0.05, err_msg=name)
        # the two ranks resume from the whole-model checkpoint (each takes its shards of m and v back), then a single process
        more = base[:-6] + ["--job-dir", str(job), "--log-every", "10", "--seed", "9"]
        (out / "resumed").mkdir()
        mp.spawn(_two_rank_trainer, args=(free_port(), more + ["--train-steps", "100"] + extra, str(out / "resumed")), nprocs=2,
                 join=True)
        a2 = torch.load(out / "resumed" / "rank0.pt")
        assert a2["step"] == 100 and (job / "model.ckpt-100.pt").exists()
        log = [json.loads(l) for l in (job / "train_log.jsonl").read_text().splitlines()]
        assert log[-1]["global_step"] == 100 and log[-1]["loss"] < log[0]["loss"]
        estimator.main(more + ["--train-steps", "110"])
        assert (job / "model.ckpt-110.pt").exists()
