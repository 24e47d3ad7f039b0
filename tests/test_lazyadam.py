"""LazyAdam on the host: the ninth optimizer name from the command line to the checkpoint, and its float64 restatement
(tests/lazyadam_ref.py) against torch.optim.SparseAdam."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import glove_ref as ref
import lazyadam_ref as lazy

GOLDEN = Path(__file__).resolve().parent / "golden"


def test_lazyadam_is_accepted_from_the_flag_to_the_checkpoint(tmp_path):
    from trainer.config_utils import parse_args
    from trainer.hip_api import GLOVE_ABI_VERSION, OPTIMIZER_CODES, DeviceTables
    from trainer.stepper import Stepper
    from trainer.train_utils import CheckpointManager, get_optimizer
    assert get_optimizer("lazyadam", learning_rate=0.01) == {
        "class_name": "LazyAdam", "config": {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "learning_rate": 0.01}}
    assert get_optimizer("LAZYADAM")["class_name"] == "LazyAdam"
    assert get_optimizer("Adam")["class_name"] == "Adam"                  # the default keeps its name and its semantics
    assert OPTIMIZER_CODES["LazyAdam"] == 8 and GLOVE_ABI_VERSION == 15
    assert "LazyAdam" in Stepper.ROWS_ONLY and "LazyAdam" not in Stepper.DENSE_ONLY
    params = parse_args(["--optimizer", "LazyAdam", "--job-dir", str(tmp_path / "job"), "--disable-datetime-path",
                         "--vocab-txt", str(GOLDEN / "text8_cov90_ctx5_vocab.txt")])
    assert params["optimizer"] == "LazyAdam"
    assert json.loads((tmp_path / "job" / "params.json").read_text())["optimizer"] == "LazyAdam"
    t = DeviceTables(12, 8, "LazyAdam", device="cpu", seed=0)
    assert sorted(t.s1) == sorted(t.s2) == ["C", "R", "bc", "br"]
    assert all(float(s.abs().max()) == 0.0 for s in list(t.s1.values()) + list(t.s2.values()))
    assert float(t.scalars.abs().max()) == 0.0
    sd = t.state_dict()
    assert sd["optimizer"] == "LazyAdam" and all("slot%d_%s" % (k, n) in sd for k in (1, 2) for n in ("R", "C", "br", "bc"))
    # a checkpoint written under LazyAdam restores under LazyAdam, both slots included ...
    for n in ("R", "C", "br", "bc"):
        t.s1[n] += 0.25
        t.s2[n] += 0.5
    t.step.fill_(7)
    CheckpointManager(str(tmp_path / "lazy")).save(t)
    fresh = DeviceTables(12, 8, "LazyAdam", device="cpu", seed=1)
    assert CheckpointManager(str(tmp_path / "lazy")).restore(fresh)
    assert fresh.global_step == 7
    for n in ("R", "C", "br", "bc"):
        assert torch.equal(getattr(fresh, n), getattr(t, n)) and torch.equal(fresh.s1[n], t.s1[n]) and torch.equal(fresh.s2[n], t.s2[n])
    # ... and the two Adams do not read each other's checkpoints: the moments mean different things
    CheckpointManager(str(tmp_path / "adam")).save(DeviceTables(12, 8, "Adam", device="cpu", seed=0))
    with pytest.raises(ValueError, match="checkpoint is for"):
        CheckpointManager(str(tmp_path / "adam")).restore(fresh)
    with pytest.raises(ValueError, match="checkpoint is for"):
        CheckpointManager(str(tmp_path / "lazy")).restore(DeviceTables(12, 8, "Adam", device="cpu", seed=0))


def test_whole_model_state_dicts_carry_both_slots():
    """load_whole_state_dict cuts a rank's rows out of a whole-model LazyAdam checkpoint, m and v included."""
    from trainer.hip_api import DeviceTables
    whole = DeviceTables(10, 4, "LazyAdam", device="cpu", seed=0)
    for k, s in enumerate((whole.s1, whole.s2)):
        for n in s:
            s[n] += torch.arange(s[n].numel(), dtype=torch.float32).reshape(s[n].shape) + 100 * k
    shard = DeviceTables(10, 4, "LazyAdam", device="cpu", seed=1, V_row=5)
    shard.load_whole_state_dict(whole.state_dict(), 2, 1)
    assert torch.equal(shard.s1["R"], whole.s1["R"][1::2]) and torch.equal(shard.s2["R"], whole.s2["R"][1::2])
    assert torch.equal(shard.s2["br"], whole.s2["br"][1::2]) and torch.equal(shard.s2["C"], whole.s2["C"])


def test_the_data_parallel_form_refuses_the_dense_exchange():
    from types import SimpleNamespace
    from trainer.stepper import RowShardedStepper, Stepper
    tables = SimpleNamespace(optimizer="LazyAdam", device=torch.device("cpu"))
    for cls in (Stepper, RowShardedStepper):
        with pytest.raises(ValueError, match="touched-rows exchange"):
            cls(SimpleNamespace(), tables, {}, 8, 2, SimpleNamespace(), exchange="dense")


# ---- the restatement against torch.optim.SparseAdam ----------------------------------------------------------------------
SA_V, SA_D, SA_STEPS, SA_LR = 11, 3, 6, 0.01


def _sparse_steps():
    """Per step: the ids of a batch with repeats (SparseAdam coalesces them, the restatement gets their sum) and one gradient
    row per occurrence, |g| in [1e-2, 1]; ids 3 and 7 never occur."""
    rng = np.random.default_rng(5)
    pool = np.array([i for i in range(SA_V) if i not in (3, 7)])
    out = []
    for _ in range(SA_STEPS):
        ids = rng.choice(pool, size=14)
        g = rng.uniform(1e-2, 1.0, (14, SA_D)) * rng.choice([-1.0, 1.0], (14, SA_D))
        out.append((ids, g))
    return out


def _formula_gap(steps):
    """The two update formulas, element by element in extended precision on this test's own gradient sums: the restatement's
    (m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; w -= lr_t m / (sqrt(v) + eps)) and torch.optim.SparseAdam's as
    torch/optim/_functional.py spells it (m += (1 - b1)(g - m); v += (1 - b2)(g^2 - v); w += -step_size m / (sqrt(v) + eps)).
    Returns the largest distance between the two parameter trajectories."""
    L = np.longdouble
    b1, b2, eps, lr = L(np.float32(0.9)), L(np.float32(0.999)), L(np.float32(1e-7)), L(np.float32(SA_LR))
    w = np.zeros((2, SA_V, SA_D), L)
    m, v = np.zeros_like(w), np.zeros_like(w)
    gap = L(0)
    for s, (ids, g) in enumerate(steps, 1):
        G = np.zeros((SA_V, SA_D), L)
        np.add.at(G, ids, g.astype(L))
        u = np.unique(ids)
        lr_t = lr * np.sqrt(1 - b2 ** s) / (1 - b1 ** s)
        m[0, u] = b1 * m[0, u] + (1 - b1) * G[u]
        v[0, u] = b2 * v[0, u] + (1 - b2) * G[u] * G[u]
        w[0, u] -= lr_t * m[0, u] / (np.sqrt(v[0, u]) + eps)
        m[1, u] += (1 - b1) * (G[u] - m[1, u])
        v[1, u] += (1 - b2) * (G[u] * G[u] - v[1, u])
        w[1, u] += -lr_t * (m[1, u] / (np.sqrt(v[1, u]) + eps))
        gap = max(gap, np.abs(w[0] - w[1]).max())
    return float(gap)


def test_restatement_equals_torch_sparse_adam():
    """Six steps, ids repeated within a batch, two ids no batch holds.  The installed torch's SparseAdam keeps epsilon beside the
    raw root and puts the bias correction into the step size — sqrt(v) + eps, lr sqrt(1 - b2^t) / (1 - b1^t) — exactly the
    restatement's formula, in another arrangement of the moment updates; gradients of at least 1e-2 keep sqrt(v) five orders of
    magnitude above epsilon, so the arrangement is all that differs.
    Tolerance, worked out here and not from what either side returns:
      * `gap`: the distance between the two formulas evaluated in extended precision on this test's gradients (printed;
        1e-18 or so: they are the same function);
      * float64 rounding: an update is bounded by |lr_t m / sqrt(v)| <= lr (1 - b1) / sqrt((1 - b2)(1 - b1^2 / b2)) = 7.3 lr
        (Cauchy-Schwarz over the two geometric weightings, lr_t <= lr), each formula spends about a dozen roundings of
        2^-53 on it, and the parameter itself rounds once per step: per step 2 x 12 x 2^-53 x 7.3 lr + 2^-53 max|w|,
        summed over the steps.
    Rows no batch touches: exactly equal, parameters and both moments exactly zero."""
    steps = _sparse_steps()
    hp = ref.Hyper(learning_rate=SA_LR)
    f32 = lambda x: float(np.float32(x))
    t = lazy.tables(SA_V, SA_D, seed=2)
    w0 = t.R.copy()
    p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SparseAdam([p], lr=f32(SA_LR), betas=(f32(0.9), f32(0.999)), eps=f32(1e-7))
    for ids, g in steps:
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids)[None, :], torch.from_numpy(g), (SA_V, SA_D))
        opt.step()
        G = np.zeros((SA_V, SA_D))
        np.add.at(G, ids, g)
        touched = np.zeros(SA_V, bool)
        touched[ids] = True
        none = np.zeros(SA_V, bool)
        gr = dict(G_R=G, touched_r=touched, G_br=np.zeros(SA_V), G_C=np.zeros((SA_V, SA_D)), G_bc=np.zeros(SA_V),
                  touched_c=none, sum_e=0.0, dg_reg=0.0)
        lazy.apply_update(t, gr, hp)
    assert t.step == SA_STEPS
    gap = _formula_gap(steps)
    ulp = 2.0 ** -53
    bound = 7.3 * f32(SA_LR)
    assert f32(SA_LR) * (1 - f32(0.9)) / math.sqrt((1 - f32(0.999)) * (1 - f32(0.9) ** 2 / f32(0.999))) <= bound
    tol = gap + SA_STEPS * (24 * ulp * bound + ulp * float(np.abs(w0).max() + SA_STEPS * bound))
    got, want = t.R, p.detach().numpy()
    err = float(np.abs(got - want).max())
    print("formula gap %.3g, tolerance %.3g, error %.3g" % (gap, tol, err))
    assert gap < 1e-16 and tol < 1e-14
    assert err <= tol
    state = opt.state[p]
    np.testing.assert_allclose(t.M_R, state["exp_avg"].numpy(), rtol=0, atol=SA_STEPS * 4 * ulp * 14)     # |G| <= 14: 14 pairs of |g| <= 1
    np.testing.assert_allclose(t.V_R, state["exp_avg_sq"].numpy(), rtol=0, atol=SA_STEPS * 4 * ulp * 14 * 14)
    for u in (3, 7):
        assert np.array_equal(got[u], w0[u]) and np.array_equal(want[u], w0[u])
        assert not t.M_R[u].any() and not t.V_R[u].any()
    assert np.abs(got - w0)[[i for i in range(SA_V) if i not in (3, 7)]].min() > 0     # every other row moved
    # the col side was given no id: nothing of it moved, only the global bias' moments (a dense variable: updated every step)
    assert not t.M_C.any() and not t.V_C.any() and float(t.M_g) == 0.0


def test_bias_correction_uses_the_global_step():
    """A row touched at steps 1 and 5 only takes, at step 5, lr_t of t = 5 (LazyAdam's definition), not of its own second update."""
    hp = ref.Hyper(learning_rate=0.01)
    t = lazy.tables(4, 2, seed=3)
    g = np.full((4, 2), 0.5)
    one = np.array([True, False, False, False])
    none = np.zeros(4, bool)
    def gr(touched):
        return dict(G_R=g, touched_r=touched, G_br=np.zeros(4), G_C=np.zeros((4, 2)), G_bc=np.zeros(4), touched_c=none, sum_e=0.0, dg_reg=0.0)
    lazy.apply_update(t, gr(one), hp)
    for _ in range(3):
        lazy.apply_update(t, gr(none), hp)
    before = t.R[0].copy()
    lazy.apply_update(t, gr(one), hp)
    b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-7))
    m = b1 * (1 - b1) * 0.5 + (1 - b1) * 0.5
    v = b2 * (1 - b2) * 0.25 + (1 - b2) * 0.25
    np.testing.assert_allclose(before - t.R[0], lazy.lr_t(hp, 5) * m / (math.sqrt(v) + eps), rtol=1e-12)
    assert t.step == 5 and lazy.lr_t(hp, 5) != lazy.lr_t(hp, 2)
