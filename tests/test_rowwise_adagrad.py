"""RowWiseAdagrad on the host: the tenth optimizer name from the command line to the checkpoint — its embedding-table slots are
float[rows], not shaped like the tables — and anchors for its float64 restatement (tests/rowwise_adagrad_ref.py) that do not
depend on the code under test: Keras-legacy Adagrad as oracle/glove_ref.py states it."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import glove_ref as ref
import rowwise_adagrad_ref as rw
from helpers import make_batch

GOLDEN = Path(__file__).resolve().parent / "golden"
NAMES = ("R", "C", "br", "bc")


def test_rowwise_adagrad_is_accepted_from_the_flag_to_the_checkpoint(tmp_path):
    from trainer.config_utils import parse_args
    from trainer.hip_api import EXPORTED_SYMBOLS, GLOVE_ABI_VERSION, OPTIMIZER_CODES, DeviceTables
    from trainer.stepper import SHARDED_OPTIMIZERS, Stepper
    from trainer.train_utils import CheckpointManager, get_optimizer
    assert get_optimizer("rowwiseadagrad", learning_rate=0.05) == {
        "class_name": "RowWiseAdagrad", "config": {"initial_accumulator_value": 0.1, "epsilon": 1e-7, "learning_rate": 0.05}}
    assert get_optimizer("ROWWISEADAGRAD")["class_name"] == "RowWiseAdagrad"
    assert get_optimizer("Adagrad")["class_name"] == "Adagrad" and get_optimizer()["class_name"] == "Adam"     # defaults stay
    with pytest.raises(ValueError, match="no HIP kernel"):
        get_optimizer("Lion")
    assert OPTIMIZER_CODES["RowWiseAdagrad"] == 9 and GLOVE_ABI_VERSION == 15 and len(EXPORTED_SYMBOLS) == 42
    assert "RowWiseAdagrad" in Stepper.ROWS_ONLY and "RowWiseAdagrad" not in Stepper.DENSE_ONLY
    assert "RowWiseAdagrad" in SHARDED_OPTIMIZERS
    params = parse_args(["--optimizer", "RowWiseAdagrad", "--job-dir", str(tmp_path / "job"), "--disable-datetime-path",
                         "--vocab-txt", str(GOLDEN / "text8_cov90_ctx5_vocab.txt")])
    assert params["optimizer"] == "RowWiseAdagrad"
    assert json.loads((tmp_path / "job" / "params.json").read_text())["optimizer"] == "RowWiseAdagrad"
    # slots: one float per row on all four variables, 0.1; the global bias' accumulator 0.1; no slot 2
    t = DeviceTables(12, 6, "RowWiseAdagrad", device="cpu", seed=0)
    assert t.d == 8 and t.R.shape == (12, 8)
    assert sorted(t.s1) == ["C", "R", "bc", "br"] and not t.s2
    for n in NAMES:
        assert t.s1[n].shape == (12,) and t.s1[n].dtype == torch.float32 and bool((t.s1[n] == np.float32(0.1)).all()), n
    assert float(t.scalars[1]) == float(np.float32(0.1)) and float(t.scalars[[0, 2, 3, 4, 5, 6, 7]].abs().max()) == 0.0
    s = t.struct()
    assert s.s1_R == t.s1["R"].data_ptr() and s.s1_C == t.s1["C"].data_ptr() and not s.s2_R and not s.s2_C
    shard = DeviceTables(12, 6, "RowWiseAdagrad", device="cpu", seed=0, V_row=5, V_col=7)
    assert shard.s1["R"].shape == (5,) and shard.s1["br"].shape == (5,) and shard.s1["C"].shape == (7,)
    # neither the twin nor the tagged form is ever set up for it
    t.enable_twin(); t.enable_tags(); t.maybe_enable_tags(64); t.maybe_enable_twin()
    assert t.R_ver is None and t.R_tag is None and t._R.shape == (12, 8)
    sd = t.state_dict()
    assert sd["optimizer"] == "RowWiseAdagrad" and sd["slot1_R"].shape == (12,) and sd["R"].shape == (12, 6)
    assert not any(k.startswith("slot2_") for k in sd)
    # a checkpoint written under RowWiseAdagrad restores under RowWiseAdagrad, the 1-D slots included ...
    for k, n in enumerate(NAMES):
        t.s1[n] += torch.arange(12, dtype=torch.float32) * (k + 1)
    t.step.fill_(7)
    CheckpointManager(str(tmp_path / "rw")).save(t)
    fresh = DeviceTables(12, 6, "RowWiseAdagrad", device="cpu", seed=1)
    assert CheckpointManager(str(tmp_path / "rw")).restore(fresh)
    assert fresh.global_step == 7
    for n in NAMES:
        assert torch.equal(getattr(fresh, n), getattr(t, n)) and torch.equal(fresh.s1[n], t.s1[n]), n
    # ... and the two Adagrads refuse each other's checkpoints, both ways: the accumulators mean different things
    CheckpointManager(str(tmp_path / "ada")).save(DeviceTables(12, 6, "Adagrad", device="cpu", seed=0))
    with pytest.raises(ValueError, match="checkpoint is for"):
        CheckpointManager(str(tmp_path / "ada")).restore(fresh)
    with pytest.raises(ValueError, match="checkpoint is for"):
        CheckpointManager(str(tmp_path / "rw")).restore(DeviceTables(12, 6, "Adagrad", device="cpu", seed=0))
    for n in NAMES:                                                     # (the refused restore wrote nothing)
        assert torch.equal(fresh.s1[n], t.s1[n]), n


class _OneRank:
    """torch.distributed of a world of one: all_gather hands the rank its own shard."""
    @staticmethod
    def all_gather(parts, x):
        parts[0].copy_(x)


def test_whole_model_state_dicts_slice_the_row_slots_by_row():
    """load_whole_state_dict cuts a rank's rows out of a whole-model checkpoint: the 1-D slots of R and C by row like br's and
    bc's, under `id % ranks` ownership and under a relabelling (--shard-balance frequency); gathered_state_dict puts a
    relabelled model back into vocabulary order."""
    from trainer.hip_api import DeviceTables
    V, d = 10, 4
    whole = DeviceTables(V, d, "RowWiseAdagrad", device="cpu", seed=0)
    for k, n in enumerate(NAMES):
        whole.s1[n] += torch.arange(V, dtype=torch.float32) + 100 * k
    sd = whole.state_dict()
    shard = DeviceTables(V, d, "RowWiseAdagrad", device="cpu", seed=1, V_row=5)
    shard.load_whole_state_dict(sd, 2, 1)
    assert torch.equal(shard.s1["R"], whole.s1["R"][1::2]) and torch.equal(shard.s1["br"], whole.s1["br"][1::2])
    assert torch.equal(shard.R, whole.R[1::2]) and torch.equal(shard.s1["C"], whole.s1["C"]) and torch.equal(shard.s1["bc"], whole.s1["bc"])
    both = DeviceTables(V, d, "RowWiseAdagrad", device="cpu", seed=1, V_row=5, V_col=5)
    both.load_whole_state_dict(sd, 2, 0)
    assert torch.equal(both.s1["C"], whole.s1["C"][0::2]) and torch.equal(both.s1["R"], whole.s1["R"][0::2])
    assert torch.equal(both.C, whole.C[0::2])
    # relabelled: token u lives in row relabel[u]; rank 1 of 2 owns rows 1, 3, 5, ...
    relabel = torch.tensor([3, 0, 7, 1, 9, 2, 8, 4, 6, 5])
    tokens = torch.empty_like(relabel)
    tokens[relabel] = torch.arange(V)
    shard = DeviceTables(V, d, "RowWiseAdagrad", device="cpu", seed=1, V_row=5)
    shard.load_whole_state_dict(sd, 2, 1, relabel=relabel)
    assert torch.equal(shard.s1["R"], whole.s1["R"][tokens][1::2]) and torch.equal(shard.R, whole.R[tokens][1::2])
    assert torch.equal(shard.s1["C"], whole.s1["C"][tokens]) and torch.equal(shard.s1["bc"], whole.s1["bc"][tokens])
    # ... and back: a relabelled one-rank model gathers into vocabulary order
    one = DeviceTables(V, d, "RowWiseAdagrad", device="cpu", seed=2)
    one.load_whole_state_dict(sd, 1, 0, relabel=relabel)
    back = one.gathered_state_dict(_OneRank, 1, relabel=relabel)
    for n in NAMES:
        assert torch.equal(back[n], sd[n]) and torch.equal(back["slot1_" + n], sd["slot1_" + n]), n
    assert back["slot1_R"].shape == (V,) and back["V_row"] == V


def test_the_multi_rank_forms_refuse_the_dense_exchange():
    from types import SimpleNamespace
    from trainer.stepper import RowShardedStepper, Stepper, sharded_exchange
    tables = SimpleNamespace(optimizer="RowWiseAdagrad", device=torch.device("cpu"))
    for cls in (Stepper, RowShardedStepper):
        with pytest.raises(ValueError, match="touched-rows exchange"):
            cls(SimpleNamespace(), tables, {}, 8, 2, SimpleNamespace(), exchange="dense")
    assert sharded_exchange(tables, "auto", True) == "rows"
    with pytest.raises(ValueError, match="eight Keras names"):
        sharded_exchange(SimpleNamespace(optimizer="Lion"), "auto", True)


# ---- anchors for the restatement: Keras-legacy Adagrad as oracle/glove_ref.py states it ---------------------------------------
def test_at_one_column_the_restatement_is_adagrad():
    """d_model = 1: the mean over one column is the square itself, so RowWiseAdagrad IS Adagrad.  Six steps on Zipf batches: the
    two float64 trajectories agree to 1e-12 on every variable, accumulator, the global bias and the loss."""
    V, B = 40, 300
    hp = ref.Hyper(learning_rate=0.05)
    a = ref.Tables(V, 1, "Adagrad", dtype=np.float32, seed=4).astype(np.float64)
    t = rw.tables(V, 1, seed=4)
    for n in NAMES:
        assert np.array_equal(getattr(t, n), getattr(a, n))
    for s in range(6):
        batch = make_batch(20 + s, B, V)
        want, got = ref.train_step(a, *batch, hp), rw.train_step(t, *batch, hp)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    for n in NAMES:
        np.testing.assert_allclose(getattr(t, n), getattr(a, n), rtol=1e-12, atol=1e-15, err_msg=n)
        np.testing.assert_allclose(getattr(t, "A_" + n).reshape(getattr(a, "A_" + n).shape), getattr(a, "A_" + n), rtol=1e-12, err_msg="A_" + n)
    np.testing.assert_allclose([t.g, t.A_g], [a.g, a.A_g], rtol=1e-12)
    assert t.step == a.step == 6 and float(np.abs(t.R - rw.tables(V, 1, seed=4).R).max()) > 1e-3          # it moved


def test_one_step_accumulates_the_row_mean_of_adagrads_increments_and_leaves_other_ids_alone():
    """From equal tables (d = 7), one step on the same batch: A_rw[u] - 0.1 == mean_j (A_adagrad[u, j] - 0.1) for every touched
    u on both sides (the same summed gradients feed both); br, bc, the global bias and their accumulators are Adagrad's own;
    the ids the batch does not hold keep W and A exactly; every touched row moved by lr G / (sqrt(A) + eps)."""
    V, d, B = 60, 7, 200
    hp = ref.Hyper(learning_rate=0.05)
    a = ref.Tables(V, d, "Adagrad", dtype=np.float32, seed=6).astype(np.float64)
    t = rw.tables(V, d, seed=6)
    t0 = t.copy()
    row, col, w, y = make_batch(31, B, V - 5)            # ids V-5 .. V-1 never occur
    gr = ref.gradients(t0, row, col, w, y, hp)
    assert np.array_equal(ref.train_step(a, row, col, w, y, hp), rw.train_step(t, row, col, w, y, hp))
    for side, ids in (("R", row), ("C", col)):
        hit = np.unique(ids)
        idle = np.setdiff1d(np.arange(V), hit)
        assert len(idle) >= 5 and len(hit) > 10
        A_rw, A_ada = getattr(t, "A_" + side), getattr(a, "A_" + side)
        np.testing.assert_allclose(A_rw[hit] - 0.1, (A_ada[hit] - 0.1).mean(1), rtol=1e-12, atol=1e-17, err_msg=side)
        G = gr["G_" + side]
        np.testing.assert_allclose(getattr(t, side)[hit], getattr(t0, side)[hit] - np.float32(0.05).astype(np.float64) * G[hit] /
                                   (np.sqrt(A_rw[hit]) + np.float64(np.float32(1e-7)))[:, None], rtol=1e-12, atol=1e-17)
        assert np.array_equal(getattr(t, side)[idle], getattr(t0, side)[idle]) and np.array_equal(A_rw[idle], getattr(t0, "A_" + side)[idle])
        assert (A_rw[hit] > 0.1).all() and (np.abs(getattr(t, side)[hit] - getattr(t0, side)[hit]).max(1) > 0).all()
        b = "br" if side == "R" else "bc"
        assert np.array_equal(getattr(t, b), getattr(a, b)) and np.array_equal(getattr(t, "A_" + b), getattr(a, "A_" + b))
        assert np.array_equal(getattr(t, b)[idle], getattr(t0, b)[idle])
    assert t.g == a.g and t.A_g == a.A_g and t.step == 1
