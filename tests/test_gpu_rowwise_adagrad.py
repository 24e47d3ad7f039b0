"""RowWiseAdagrad (GLOVE_OPT_ROWWISE_ADAGRAD: one Adagrad accumulator per embedding row, fed by the row's mean squared gradient)
on the GPU, held to its float64 restatement (tests/rowwise_adagrad_ref.py) at every kernel shape and plan kind
tests/test_gpu_optimizer_matrix.py runs the per-row optimizers at — its case lists are imported, its tolerances apply: loss rtol
2e-5; one step rtol 1e-5 / atol 1e-6; trajectories 5e-5 / 5e-6.

  shapes (1 + 20 steps)   heavy ids   edge shapes   device-refilled plans   untouched rows and accumulators bit for bit
  padding columns   captured and replayed   the touched-rows exchange and the sharded forms on one rank   the trainer end to
  end   argument errors"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import glove_ref as ref
import rowwise_adagrad_ref as rw
from helpers import free_port, make_batch, to_dev
from rowwise_adagrad_ref import assert_tables_close
from test_gpu_optimizer_matrix import (EDGE_CASES, HEAVY, KEY, LOSS_RTOL, REFILLED, ROWS_SHAPES, SHAPE_IDS, SHAPES, STEP_TOL, TRAJ_TOL,
                                       _heavy_batch)

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden"
LR = 0.05                   # (Adagrad's learning rate in this suite: test_gpu_optimizers.CASES gives it to Ftrl, the other
                            # accumulator optimizer, and test_gpu_optimizer_matrix / smoke() step Adagrad itself with it)
NAMES = ("R", "C", "br", "bc")


def _hyper(B, **extra):
    from trainer.hip_api import make_hyper
    hp = ref.Hyper(learning_rate=LR)
    return hp, make_hyper(l2_reg=hp.l2_reg, reg_mult=hp.reg_mult, learning_rate=LR, batch_size=B, optimizer="RowWiseAdagrad", **extra)


def _steps(hip, dt, t, h, hp, batches, V, cap, tol_first, tol_end):
    """One step per batch on the device and in the restatement: the loss after every step, the whole state after the first and
    the last.  No dense buffer is handed over: the step must not want one."""
    loss_out = torch.zeros(4, device="cuda:0")
    plans = []
    for s, (row, col, w, y) in enumerate(batches):
        plan = hip.build_plan(*to_dev(row, col, w, y), V, chunk_cap=cap)
        plans.append(plan)
        hip.step_sparse(plan, dt, h, None, loss_out)
        want = rw.train_step(t, row, col, w, y, hp)
        np.testing.assert_allclose(loss_out.cpu().numpy()[:3], want, rtol=LOSS_RTOL, err_msg="loss of step %d" % s)
        if s == 0 and len(batches) > 1:
            assert_tables_close(dt, t, *tol_first)
    assert_tables_close(dt, t, *(tol_end if len(batches) > 1 else tol_first))
    return plans


@pytest.mark.parametrize("B,V,d,cap,stride", SHAPES, ids=SHAPE_IDS)
def test_every_kernel_shape_one_step_and_twenty(hip, B, V, d, cap, stride):
    """One step, then twenty on fresh batches, at every (lanes-per-row, float4-per-lane) shape; the id no batch holds keeps its
    row and its accumulators bit for bit (the padding columns of R and C exactly zero: assert_tables_close)."""
    from trainer.hip_api import DeviceTables
    hp, h = _hyper(B)
    t = rw.tables(V, d)
    dt = rw.device_tables(t, DeviceTables)
    assert dt.d == stride and dt.optimizer == "RowWiseAdagrad"
    keep = V - 1
    before = rw.snapshot(dt)
    batches = [make_batch(700 + 13 * s + d, B, V - 1) for s in range(21)]
    _steps(hip, dt, t, h, hp, batches, V, cap, STEP_TOL, TRAJ_TOL)
    after = rw.snapshot(dt)
    for k in before:
        if k not in ("scalars", "step"):
            assert torch.equal(after[k][keep], before[k][keep]), k
    assert dt.global_step == 21


@pytest.mark.parametrize("name,B,V,d,cap", HEAVY, ids=[c[0] for c in HEAVY])
def test_heavy_ids(hip, name, B, V, d, cap):
    """Ids of more than HEAVY_CHUNKS chunks (a whole workgroup reduces them), two steps as the matrix runs them."""
    from trainer.hip_api import DeviceTables
    hp, h = _hyper(B)
    t = rw.tables(V, d)
    dt = rw.device_tables(t, DeviceTables)
    if cap == 1:
        batches = [make_batch(90 + s, B, V) for s in range(2)]
    else:
        row, col, w, y = _heavy_batch(B, V)
        batches = [(row, col, w, y), (row, col, w * np.float32(1.1), y)]
    plans = _steps(hip, dt, t, h, hp, batches, V, cap, TRAJ_TOL, TRAJ_TOL)
    for p in plans:
        assert p.compact().host_counts[4] > 0, "the batch holds no heavy id"


@pytest.mark.parametrize("B,V,d,cap", EDGE_CASES)
def test_edge_shapes(hip, B, V, d, cap):
    """The degenerate shapes of test_gpu_parity.EDGE_CASES, two steps on the same batch (tolerances of the matrix's case C)."""
    from trainer.hip_api import DeviceTables
    row, col, w, y = make_batch(B + 5 * V + d, B, V, zipf=(V > 3))
    if V == 4096:                                       # every id exactly once on each side
        row = np.random.default_rng(0).permutation(V).astype(np.int32)
        col = ((row.astype(np.int64) * 7 + 1) % V).astype(np.int32)
    hp, h = _hyper(B)
    t = rw.tables(V, d)
    dt = rw.device_tables(t, DeviceTables)
    _steps(hip, dt, t, h, hp, [(row, col, w, y)] * 2, V, cap, STEP_TOL, (2e-5, 2e-6))


@pytest.mark.parametrize("records", [True, False], ids=["records", "pair-arrays"])
@pytest.mark.parametrize("name,V,d,B,cap", REFILLED, ids=[c[0] for c in REFILLED])
def test_device_refilled_plans(hip, name, V, d, B, cap, records):
    """What --epoch-shuffle full feeds the step: masters -> deal -> glove_plan_build_sorted into staging plans, with chunk
    records and with pair arrays.  Every step == the step on glove_plan_build of the same batch, and on that plan compacted,
    bit for bit; the end state == the restatement."""
    from trainer.hip_api import DeviceTables, Pairs, PlanBlock
    n = 3 * B + 77
    row, col, w, y = make_batch(V + d, n, V)
    if name == "heavy":
        row[np.random.default_rng(5).random(n) < 0.6] = 3
        col[row == col] = (col[row == col] + 1) % V
    m = hip.build_masters(*to_dev(row, col, w, y), V)
    rs, cs = Pairs(n, "cuda:0"), Pairs(n, "cuda:0")
    hip.deal_epoch(m, B, KEY, rs, cs, hip.deal_workspace(n, B, "cuda:0"))
    nb = n // B
    block = PlanBlock([hip.staging_plan(B, V, cap, "cuda:0", records=records) for _ in range(nb)])
    ws = torch.empty(hip.lib.glove_plan_sorted_workspace_bytes(B, nb), dtype=torch.uint8, device="cuda:0")
    hip.build_plans_sorted(rs, cs, 0, block, nb, V, ws)
    hp, h = _hyper(B)
    t = rw.tables(V, d)
    tabs = [rw.device_tables(t, DeviceTables) for _ in range(3)]
    losses = [torch.zeros(4, device="cuda:0") for _ in range(3)]
    for k in range(nb):
        staged = block.plans[k]
        assert staged.host_counts[4] < 0 and (staged.r_crec is not None) == records
        arrays = [a.contiguous() for a in rs.arrays(k * B, (k + 1) * B)]
        built = hip.build_plan(*arrays, V, chunk_cap=cap, records=records or None, links=False, run_words=False)
        exact = built.compact(hip.lib)
        for plan, x, lo in zip((staged, built, exact), tabs, losses):
            hip.step_sparse(plan, x, h, None, lo)
        assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2]), (k, [lo.tolist() for lo in losses])
        rw.train_step(t, *(a.cpu().numpy() for a in arrays), hp)
    first = rw.snapshot(tabs[0])
    for other in tabs[1:]:
        rw.assert_bitwise_equal(first, rw.snapshot(other), name)
    assert_tables_close(tabs[0], t, *TRAJ_TOL)


def test_untouched_rows_and_accumulators_keep_their_bits(hip):
    """V = 4096, B = 256, d = 64: after a step every row whose id is not in the batch has W and A bitwise unchanged on both
    tables and both bias vectors; every touched row moved, no touched accumulator shrank and some grew; the global bias and its accumulator changed."""
    from trainer.hip_api import DeviceTables, make_hyper
    V, B, d = 4096, 256, 64
    row, col, w, y = make_batch(9, B, V)
    plan = hip.build_plan(*to_dev(row, col, w, y), V)
    idle = {"R": np.setdiff1d(np.arange(V), row), "C": np.setdiff1d(np.arange(V), col)}
    assert len(idle["R"]) > V - B - 1 and len(idle["C"]) > V - B - 1
    dt = DeviceTables(V, d, "RowWiseAdagrad", device="cuda:0", seed=4)
    gen = torch.Generator(device="cpu").manual_seed(17)
    for n in NAMES:                                     # accumulators mid-run: a different value in every row
        dt.s1[n].copy_(0.1 + torch.rand(dt.s1[n].shape[0], generator=gen))
    dt.step.fill_(40)
    before = {n: (getattr(dt, n).clone(), dt.s1[n].clone()) for n in NAMES}
    scalars = dt.scalars.clone()
    h = make_hyper(learning_rate=LR, batch_size=B, optimizer="RowWiseAdagrad")
    loss_out = torch.zeros(4, device="cuda:0")
    hip.step_sparse(plan, dt, h, None, loss_out)
    torch.cuda.synchronize()
    assert dt.global_step == 41 and np.isfinite(loss_out.cpu().numpy()).all()
    assert all(float(dt.scalars[k]) != float(scalars[k]) for k in range(2)), "global bias / its accumulator did not move"
    assert torch.equal(dt.scalars[2:], scalars[2:])
    for n in NAMES:
        ids = torch.from_numpy(idle["R" if n in ("R", "br") else "C"]).cuda()
        hit = torch.from_numpy(np.unique(row if n in ("R", "br") else col)).cuda().long()
        for what, now, was in zip(("W", "A"), (getattr(dt, n), dt.s1[n]), before[n]):
            assert torch.equal(now[ids], was[ids]), "untouched rows of %s moved (%s)" % (n, what)
        diff = getattr(dt, n)[hit] != before[n][0][hit]
        assert bool(diff.reshape(len(hit), -1).any(1).all()), "a touched row of %s did not move" % n
        # (an accumulator of 0.1 .. 1.1 has an ulp of up to 1.2e-7: the mean squared gradient of a cold id with one light pair
        # lies below it — how far each one moves is the trajectory tests' business; here: none shrinks, and some grow)
        grew = dt.s1[n][hit] - before[n][1][hit]
        assert bool((grew >= 0).all()) and float(grew.max()) > 0, "accumulators of touched rows of %s: %s" % (n, grew[:8].tolist())


def test_padding_columns_stay_exactly_zero_over_twenty_steps(hip):
    """d_model = 50 in rows of 52 floats: after twenty steps the two padding columns of R and C hold exactly 0.0f (their G is 0
    and takes no share of the row's mean: the mean is over d_model = 50, which the restatement's accumulators confirm)."""
    from trainer.hip_api import DeviceTables
    B, V, d, cap = 1024, 300, 50, 32
    hp, h = _hyper(B)
    t = rw.tables(V, d)
    dt = rw.device_tables(t, DeviceTables)
    assert dt.d == 52 and dt.d_model == 50
    _steps(hip, dt, t, h, hp, [make_batch(40 + s, B, V) for s in range(20)], V, cap, STEP_TOL, TRAJ_TOL)
    for n in ("R", "C"):
        pad = getattr(dt, n)[:, 50:]
        assert pad.shape == (V, 2) and bool((pad.contiguous().view(torch.int32) == 0).all()), n + " padding is not +0.0"


def test_four_steps_captured_and_replayed_twice_equal_eight_eager_steps(hip):
    """The row reduction has a fixed order and nothing of a step lives on the host: a hipGraph of four steps, replayed twice,
    is bit for bit the eight eager steps."""
    from trainer.hip_api import DeviceTables
    B, V, d = 1024, 300, 64
    hp, h = _hyper(B)
    t = rw.tables(V, d)
    a, b = rw.device_tables(t, DeviceTables), rw.device_tables(t, DeviceTables)
    batches = [make_batch(50 + s, B, V) for s in range(4)]
    plans = [hip.build_plan(*to_dev(*bt), V) for bt in batches]
    la, lb = torch.zeros(4, device="cuda:0"), torch.zeros(4, device="cuda:0")
    ws = torch.empty(max(hip.lib.glove_step_workspace_bytes(B, p.cap_chunks, a.d) for p in plans), dtype=torch.uint8, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm the launch path outside the capture (one step on both)
        hip.step_sparse(plans[3], a, h, None, la, ws)
        hip.step_sparse(plans[3], b, h, None, lb, ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for p in plans:
            hip.step_sparse(p, a, h, None, la, ws)
    for _ in range(2):
        g.replay()
    for _ in range(2):
        for p in plans:
            hip.step_sparse(p, b, h, None, lb, ws)
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 9
    rw.assert_bitwise_equal(rw.snapshot(a), rw.snapshot(b), "replayed vs eager")
    assert torch.equal(la, lb)
    for k in (3, 0, 1, 2, 3, 0, 1, 2, 3):               # ... and both are the restatement's nine steps
        rw.train_step(t, *batches[k], hp)
    assert_tables_close(a, t, *TRAJ_TOL)
    del g


@pytest.mark.parametrize("B,V,d,cap", ROWS_SHAPES, ids=["d%d-B%d-V%d" % (s[2], s[0], s[1]) for s in ROWS_SHAPES])
def test_touched_rows_exchange_on_one_rank(hip, B, V, d, cap):
    """Stepper(exchange="rows") on one rank (pack -> copy -> combine -> apply_packed_kernel) against glove_step_sparse_f32 on
    the same plan and against the restatement, three steps: bit for bit where the packing passes sum every id chunk by chunk
    like the plain passes (no chunk records, or one chunk per id), within rtol 2e-5 elsewhere; the marks come back all zero."""
    from trainer.hip_api import DeviceTables
    from trainer.stepper import HipBackend, Stepper
    row, col, w, y = _heavy_batch(B, V) if V == 40 else make_batch(77 + d, B, V)
    hp = ref.Hyper(learning_rate=LR)
    t = rw.tables(V, d)
    tabs = [rw.device_tables(t, DeviceTables) for _ in range(2)]
    backend = HipBackend("cuda:0")
    plan = hip.build_plan(*to_dev(row, col, w, y), V, chunk_cap=cap, compact=True)
    kw = dict(l2_reg=hp.l2_reg, reg_mult=hp.reg_mult, learning_rate=LR, optimizer="RowWiseAdagrad")
    rows, plain = Stepper(backend, tabs[0], kw, B, exchange="rows"), Stepper(backend, tabs[1], kw, B)
    rows.prepare([plan])
    plain.prepare([plan])
    assert rows.rows and [n for n, _ in rows.phases()] == ["passes", "pack_grad", "all_gather", "combine_apply"]
    assert [n for n, _ in plain.phases()] == ["step"] and plain.G is None and plain._rms_G is None
    assert tabs[1].R_tag is None and tabs[1].R_ver is None          # neither the tagged nor the twin form is set up for it
    rows.G.fill_(float("nan"))                        # whatever the buffer holds: first touches store, they do not add
    for _ in range(3):
        rows.step(plan)
        plain.step(plan)
        want = rw.train_step(t, row, col, w, y, hp)
        assert int(rows.bufs["mark"].abs().max()) == 0
    got, ref_ = rw.snapshot(tabs[0]), rw.snapshot(tabs[1])
    if plan.r_crec is None or plan.host_counts[6] == 1:
        rw.assert_bitwise_equal(got, ref_, "rows vs plain")
        assert torch.equal(rows.loss_out[:3], plain.loss_out[:3])
    else:
        for k in got:
            if k != "step":
                torch.testing.assert_close(got[k][:3] if k == "scalars" else got[k], ref_[k][:3] if k == "scalars" else ref_[k],
                                           rtol=2e-5, atol=2e-6, msg=lambda m: k + ": " + m)
        torch.testing.assert_close(rows.loss_out[:3], plain.loss_out[:3], rtol=2e-5, atol=0)
    np.testing.assert_allclose(rows.loss_out.cpu().numpy()[:3], want, rtol=LOSS_RTOL)
    for x in tabs:
        assert_tables_close(x, t, *TRAJ_TOL)


def test_sharded_forms_through_rccl_with_one_rank(hip):
    """Row-sharded with the lists and both tables sharded, every collective through RCCL on this one GPU (a process group of one
    rank, the fully sharded form's exchange exercised: glove_rowside_step_f32 on the row side, the owner's packed apply on the
    col side): each equals the plain single-GPU step_sparse run — the tolerances of tests/test_gpu_sharded_optimizers.py —
    and the row-sharded form refuses the dense col exchange."""
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
        t = rw.tables(V, d, seed=5)
        kw = dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.01, optimizer="RowWiseAdagrad")
        plain_t = rw.device_tables(t, DeviceTables)
        plain = Stepper(backend, plain_t, kw, B)
        with pytest.raises(ValueError, match="touched-rows exchange"):
            RowShardedStepper(backend, rw.device_tables(t, DeviceTables), kw, B, 1, dist, exchange="dense", collectives=True)
        runs = {}
        tabs = rw.device_tables(t, DeviceTables)
        st = RowShardedStepper(backend, tabs, kw, B, 1, dist, exchange="auto", collectives=True)
        st.prepare(plans)
        assert st.rows and "rowside_step" in [n for n, _ in st.phases()]
        runs["row-sharded, rows"] = (tabs, st, plans)
        tabs = rw.device_tables(t, DeviceTables)
        st = ShardedStepper(backend, tabs, kw, B, 1, 0, dist, collectives=True, exercise_exchange=True)
        runs["both tables sharded"] = (tabs, st, [st.add_batch(*bt) for bt in batches])
        hp = ref.Hyper(learning_rate=0.01)
        for s in range(steps):
            plain.step(plans[s])
            for tabs, st, items in runs.values():
                st.step(items[s])
            rw.train_step(t, *(x.cpu().numpy() for x in batches[s]), hp)
        want = rw.snapshot(plain_t)
        for name, (tabs, st, _) in runs.items():
            got = rw.snapshot(tabs)
            assert int(got["step"]) == int(want["step"]) == steps, name
            for k in want:
                if k == "step":
                    continue
                a, b = (got[k][:3], want[k][:3]) if k == "scalars" else (got[k], want[k])
                torch.testing.assert_close(a, b, rtol=2e-5, atol=2e-6, msg=lambda m: "%s %s: %s" % (name, k, m))
            np.testing.assert_allclose(st.read_loss()["loss"], plain.read_loss()["loss"], rtol=2e-5, err_msg=name)
            assert_tables_close(tabs, t, *TRAJ_TOL)
        assert_tables_close(plain_t, t, *TRAJ_TOL)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("shuffle", ["static", "full"])
def test_trainer_end_to_end(hip, tmp_path, shuffle):
    """`python -m trainer.estimator --optimizer rowwiseadagrad` on the golden text8 fixture, both epoch modes: it trains (the eval
    loss over the whole file falls), the checkpoint holds one accumulator per row and no second slot, and a second invocation
    resumes from it to a later max_steps."""
    csv, vocab = GOLDEN / "text8_cov90_ctx5_interaction.csv", GOLDEN / "text8_cov90_ctx5_vocab.txt"
    job = tmp_path / "job"
    base = [sys.executable, "-m", "trainer.estimator", "--train-csv", str(csv), "--vocab-txt", str(vocab), "--job-dir", str(job),
            "--disable-datetime-path", "--embedding-size", "16", "--optimizer", "rowwiseadagrad", "--learning-rate", "0.05",
            "--batch-size", "64", "--log-every", "50", "--seed", "3", "--epoch-shuffle", shuffle, "--save-checkpoints-secs", "0"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(HERE.parent)] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    for steps in (200, 300):
        proc = subprocess.run(base + ["--train-steps", str(steps)], cwd=str(HERE.parent), env=env, capture_output=True, text=True,
                              timeout=240)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
        # (read before the next invocation: a reshuffled run saves at every epoch's and burst's end, and only the last five stay)
        blob = torch.load(job / ("model.ckpt-%d.pt" % steps), weights_only=False)["tables"]
        assert blob["optimizer"] == "RowWiseAdagrad" and int(blob["global_step"]) == steps
        for n in NAMES:
            a = blob["slot1_" + n]
            assert a.shape == (blob["V"],) and "slot2_" + n not in blob, n
            assert float(a.min()) >= float(np.float32(0.1)) and float(a.max()) > 0.1, n
        assert blob["R"].shape == (blob["V"], 16)
    ev = [json.loads(l) for l in (job / "eval" / "eval_log.jsonl").read_text().splitlines()]
    steps_seen = [e["global_step"] for e in ev]
    assert steps_seen[-1] == 300 and 200 in steps_seen and steps_seen == sorted(steps_seen)
    at200 = [e for e in ev if e["global_step"] == 200][0]
    assert at200["average_loss"] < ev[0]["average_loss"] and ev[-1]["average_loss"] < ev[0]["average_loss"]
    log = [json.loads(l) for l in (job / "train_log.jsonl").read_text().splitlines()]
    later = [r["global_step"] for r in log if r["global_step"] > 200]
    assert later and later[-1] == 300 and len(log) - len(later) >= 1          # the second run went on from 200, not from 0
    assert sum(r["global_step"] <= 50 for r in log) == 1                       # (step 50 was logged once: nothing was trained twice)


def test_argument_errors(hip):
    """glove_dense_adam_f32 and glove_dense_adagrad_f32 refuse the new code (no sweep can walk float[rows] slots); a NULL s1_R is
    refused by the step and by the row side's step before anything is launched: the tables keep their bits."""
    import ctypes as C
    from trainer.hip_api import GloveHipError, OPTIMIZER_CODES, DeviceTables, make_hyper
    B, V, d = 256, 100, 16
    dt = DeviceTables(V, d, "RowWiseAdagrad", device="cuda:0", seed=0)
    plan = hip.build_plan(*to_dev(*make_batch(3, B, V)), V)
    h = make_hyper(learning_rate=LR, batch_size=B, optimizer="RowWiseAdagrad")
    assert h.optimizer == OPTIMIZER_CODES["RowWiseAdagrad"] == 9
    before = rw.snapshot(dt)
    G = hip.dense_grad_buffer(dt)
    st = torch.cuda.current_stream().cuda_stream
    assert hip.lib.glove_dense_adam_f32(C.byref(dt.struct()), C.byref(h), G.data_ptr(), None, st) == -1
    assert hip.lib.glove_dense_adagrad_f32(C.byref(dt.struct()), C.byref(h), G.data_ptr(), None, st) == -1
    with pytest.raises(GloveHipError, match="GLOVE_E_BADARG"):
        hip.dense_adam(dt, h, G)
    bad = type(dt.struct()).from_buffer_copy(dt.struct())
    bad.s1_R = None
    ws = hip.step_workspace(plan, dt.d)
    assert hip.lib.glove_step_sparse_f32(C.byref(plan.struct()), C.byref(bad), C.byref(h), ws.data_ptr(), ws.numel(), None, None, st) == -1
    hr = make_hyper(learning_rate=LR, batch_size=B, optimizer="RowWiseAdagrad", sides=1)
    assert hip.lib.glove_rowside_step_f32(C.byref(plan.struct()), C.byref(bad), C.byref(hr), ws.data_ptr(), ws.numel(), None, st) == -1
    torch.cuda.synchronize()
    rw.assert_bitwise_equal(before, rw.snapshot(dt), "after refused calls")
    loss_out = torch.zeros(4, device="cuda:0")
    hip.step_sparse(plan, dt, h, None, loss_out)              # ... and the same arguments with the slot in place step
    assert dt.global_step == 1 and np.isfinite(loss_out.cpu().numpy()).all()
