"""The six optimizers with kernels of their own (SGD plain / momentum / Nesterov, RMSprop, Adamax, Adadelta, Ftrl, Nadam:
glove_step_sparse_f32 -> apply_sparse_opt_kernel, nadam_fused_kernel, dense_rmsprop_kernel; on the touched-rows exchange
apply_packed_kernel) held to the float64 oracle (oracle/glove_ref.py) at every (lanes-per-row, float4-per-lane) kernel shape,
on heavy ids, at edge shapes, from a loaded mid-run state, and on the device-refilled plans of a reshuffled epoch; and the
one-launch (tagged) Adagrad and Adam steps on a dealt batch that holds a heavy id.

  A  every kernel shape            B  heavy ids (the workgroup path)   C  edge shapes
  D  mid-run state, large step     E  device-refilled plans            F  touched-rows exchange on one GPU
  G  tagged form on a dealt heavy batch (Adagrad, Adam)
  H  GloveHip.step == the name's own wrapper, bit for bit (every name)

Tolerances (those of test_gpu_optimizers.py): loss rtol 2e-5; one step rtol 1e-5 / atol 1e-6; trajectories 5e-5 / 5e-6.
In every case the padding columns of R and C stay exactly zero, those of every slot at their initial value, global_step
is right, and the dense buffer of RMSprop and Nadam is all zero again."""
import numpy as np
import pytest
import torch

import glove_ref as ref
from helpers import assert_opt_tables_close, make_batch, opt_tables_from_oracle, oracle_tables, to_dev
from test_gpu_optimizers import CASES as CONFIGS
from test_gpu_parity import EDGE_CASES

gpu = pytest.mark.gpu
CONFIG_IDS = ["SGD", "SGD-momentum", "SGD-nesterov", "RMSprop", "Adamax", "Adadelta", "Ftrl", "Nadam"]
LOSS_RTOL = 2e-5
STEP_TOL = (1e-5, 1e-6)
TRAJ_TOL = (5e-5, 5e-6)
KEY = 0x0123456789abcdef_fedcba9876543210

# (B, V, d_model, chunk_cap, row stride): the stride picks the kernel shape (glove_common.h pick_pass_shape / pick_row_shape)
SHAPES = [
    (7, 50, 1, 32, 4),              # pass 8x1, rows 16x1
    (1024, 300, 50, 32, 52),        # pass 8x2, rows 16x1
    (1024, 120, 100, 16, 100),      # 32x1
    (2048, 400, 150, 8, 160),       # 64x1
    (900, 70, 301, 7, 304),         # 32x3
    (2048, 64, 500, 32, 512),       # 64x2
    (512, 64, 700, 16, 704),        # 64x3
    (2048, 64, 1024, 32, 1024),     # 64x4
    (30000, 300000, 128, 16, 128),  # 32x1, many ids
]
SHAPE_IDS = ["d%d-B%d-V%d" % (s[2], s[0], s[1]) for s in SHAPES]


def _hyper(optimizer, kw, lr, B, **extra):
    from trainer.hip_api import make_hyper
    hp = ref.Hyper(learning_rate=lr, **kw)
    return hp, make_hyper(l2_reg=hp.l2_reg, reg_mult=hp.reg_mult, learning_rate=lr, batch_size=B, optimizer=optimizer, **kw, **extra)


def _dense_buffer(hip, dt):
    return hip.dense_grad_buffer(dt) if dt.optimizer in ("RMSprop", "Nadam") else None


def _assert_buffer_zero(G):
    if G is not None:
        assert float(G.abs().max()) == 0.0, "the dense buffer is not all zero again"


def _heavy_batch(B, V):
    """The batch of test_gpu_parity.test_heavy_ids_take_the_workgroup_path: 70 % of the rows id 3, half the cols id 7."""
    rng = np.random.default_rng(2)
    row = np.where(rng.random(B) < 0.7, 3, rng.integers(0, V, B)).astype(np.int32)
    col = np.where(rng.random(B) < 0.5, 7, rng.integers(0, V, B)).astype(np.int32)
    col[row == col] = (col[row == col] + 1) % V
    _, _, w, y = make_batch(4, B, V)
    return row, col, w, y


def _steps(hip, dt, t, h, hp, batches, V, cap, tol_first, tol_end, G=None):
    """One step per batch on the device and in the oracle: the loss after every step, the whole state after the first and the last."""
    loss_out = torch.zeros(4, device="cuda:0")
    plans = []
    for s, (row, col, w, y) in enumerate(batches):
        plan = hip.build_plan(*to_dev(row, col, w, y), V, chunk_cap=cap)
        plans.append(plan)
        hip.step_sparse(plan, dt, h, G, loss_out)
        want = ref.train_step(t, row, col, w, y, hp)
        np.testing.assert_allclose(loss_out.cpu().numpy()[:3], want, rtol=LOSS_RTOL, err_msg="loss of step %d" % s)
        if s == 0 and len(batches) > 1:
            assert_opt_tables_close(dt, t, *tol_first)
    assert_opt_tables_close(dt, t, *(tol_end if len(batches) > 1 else tol_first))
    _assert_buffer_zero(G)
    return plans


@pytest.mark.parametrize("B,V,d,cap,stride", SHAPES, ids=SHAPE_IDS)
def test_row_width_keeps_every_shape_case_on_its_stride(B, V, d, cap, stride):
    """The strides the shape cases below were chosen for: a change to row_width must not move a case off its kernel shape."""
    from trainer.hip_api import row_width
    assert row_width(V, d) == stride


# ---- A: every kernel shape ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,V,d,cap,stride", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("optimizer,kw,lr", CONFIGS, ids=CONFIG_IDS)
def test_a_every_kernel_shape(hip, optimizer, kw, lr, B, V, d, cap, stride):
    """One step, then five on fresh batches; the id no batch holds does not move (RMSprop, Nadam: only its slots decay)."""
    from trainer.hip_api import DeviceTables
    hp, h = _hyper(optimizer, kw, lr, B)
    t = oracle_tables(V, d, optimizer)
    dt = opt_tables_from_oracle(t, DeviceTables)
    assert dt.d == stride
    keep = V - 1
    r0, c0, br0, bc0 = dt.R[keep].clone(), dt.C[keep].clone(), dt.br[keep].clone(), dt.bc[keep].clone()
    batches = [make_batch(700 + 13 * s + d, B, V - 1) for s in range(6)]
    _steps(hip, dt, t, h, hp, batches, V, cap, STEP_TOL, TRAJ_TOL, _dense_buffer(hip, dt))
    assert torch.equal(dt.R[keep], r0) and torch.equal(dt.C[keep], c0)
    assert torch.equal(dt.br[keep], br0) and torch.equal(dt.bc[keep], bc0)


# ---- B: heavy ids -------------------------------------------------------------------------------------------------------
HEAVY = [("heavy-d64", 30000, 40, 64, 8), ("heavy-d301", 30000, 40, 301, 8), ("heavy-d1024", 30000, 40, 1024, 8),
         ("cap1-d128", 20000, 300, 128, 1)]


@gpu
@pytest.mark.parametrize("name,B,V,d,cap", HEAVY, ids=[c[0] for c in HEAVY])
@pytest.mark.parametrize("optimizer,kw,lr", CONFIGS, ids=CONFIG_IDS)
def test_b_heavy_ids(hip, optimizer, kw, lr, name, B, V, d, cap):
    """Ids of more than HEAVY_CHUNKS chunks are reduced by a whole workgroup (for_each_id's heavy blocks); two steps (the
    tolerance of a trajectory: an id of 21,000 pairs sums them in fp32)."""
    from trainer.hip_api import DeviceTables
    hp, h = _hyper(optimizer, kw, lr, B)
    t = oracle_tables(V, d, optimizer)
    dt = opt_tables_from_oracle(t, DeviceTables)
    if cap == 1:
        batches = [make_batch(90 + s, B, V) for s in range(2)]
    else:
        row, col, w, y = _heavy_batch(B, V)
        batches = [(row, col, w, y), (row, col, w * np.float32(1.1), y)]
    plans = _steps(hip, dt, t, h, hp, batches, V, cap, TRAJ_TOL, TRAJ_TOL, _dense_buffer(hip, dt))
    for p in plans:
        assert p.compact().host_counts[4] > 0, "the batch holds no heavy id"


# ---- C: edge shapes -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,V,d,cap", EDGE_CASES)
@pytest.mark.parametrize("optimizer,kw,lr", CONFIGS, ids=CONFIG_IDS)
def test_c_edge_shapes(hip, optimizer, kw, lr, B, V, d, cap):
    """The degenerate shapes of test_gpu_parity.EDGE_CASES, two steps on the same batch (the tolerance of the Adagrad case)."""
    from trainer.hip_api import DeviceTables
    row, col, w, y = make_batch(B + 5 * V + d, B, V, zipf=(V > 3))
    if V == 4096:                                       # every id exactly once on each side
        row = np.random.default_rng(0).permutation(V).astype(np.int32)
        col = ((row.astype(np.int64) * 7 + 1) % V).astype(np.int32)
    hp, h = _hyper(optimizer, kw, lr, B)
    t = oracle_tables(V, d, optimizer)
    dt = opt_tables_from_oracle(t, DeviceTables)
    _steps(hip, dt, t, h, hp, [(row, col, w, y)] * 2, V, cap, STEP_TOL, (2e-5, 2e-6), _dense_buffer(hip, dt))


# ---- D: mid-run state at a large global_step ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("step", [1000, 1000000])
@pytest.mark.parametrize("optimizer,kw,lr", CONFIGS, ids=CONFIG_IDS)
def test_d_from_a_loaded_mid_run_state(hip, optimizer, kw, lr, step):
    """Twenty oracle steps move every slot (Ftrl's z and n, Nadam's momentum cache, Adamax's m and v); global_step then jumps
    to `step` (Adamax's lr_t = lr / (1 - beta1^t) in fp32 through expm1f, Nadam's schedule and cache parity); the whole state
    goes into the device tables and both sides take three more steps."""
    from trainer.hip_api import DeviceTables
    B, V, d, cap = 2048, 400, 150, 8
    hp, h = _hyper(optimizer, kw, lr, B)
    t = oracle_tables(V, d, optimizer)
    for s in range(20):
        ref.train_step(t, *make_batch(300 + s, B, V), hp)
    t = t.astype(np.float32).astype(np.float64)      # the state the device can hold exactly
    t.step = step
    if optimizer == "Nadam":
        assert t.m_cache < 0.01                       # (twenty steps of the schedule: the cache is far from its initial 1)
    dt = opt_tables_from_oracle(t, DeviceTables)
    assert_opt_tables_close(dt, t, 0, 0)
    _steps(hip, dt, t, h, hp, [make_batch(400 + s, B, V) for s in range(3)], V, cap, STEP_TOL, TRAJ_TOL, _dense_buffer(hip, dt))
    assert dt.global_step == step + 3


# ---- E: device-refilled plans of a dealt epoch --------------------------------------------------------------------------
REFILLED = [("small", 300, 64, 1024, 32), ("wide", 10000, 300, 16384, 32), ("heavy", 40, 64, 8192, 8)]


@gpu
@pytest.mark.parametrize("records", [True, False], ids=["records", "pair-arrays"])
@pytest.mark.parametrize("name,V,d,B,cap", REFILLED, ids=[c[0] for c in REFILLED])
@pytest.mark.parametrize("optimizer,kw,lr", CONFIGS, ids=CONFIG_IDS)
def test_e_device_refilled_plans(hip, optimizer, kw, lr, name, V, d, B, cap, records):
    """What --epoch-shuffle full feeds these optimizers: masters -> deal -> glove_plan_build_sorted into staging plans (host
    counts unknown: the step sizes its heavy blocks by cap_heavy).  Every step == the step on glove_plan_build of the same
    batch, and on that plan compacted (exact heavy blocks), bit for bit; the end state == the oracle."""
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
    hp, h = _hyper(optimizer, kw, lr, B)
    t = oracle_tables(V, d, optimizer)
    tabs = [opt_tables_from_oracle(t, DeviceTables) for _ in range(3)]
    Gs = [_dense_buffer(hip, x) for x in tabs]
    losses = [torch.zeros(4, device="cuda:0") for _ in range(3)]
    for k in range(nb):
        staged = block.plans[k]
        assert staged.host_counts[4] < 0 and (staged.r_crec is not None) == records
        arrays = [a.contiguous() for a in rs.arrays(k * B, (k + 1) * B)]
        built = hip.build_plan(*arrays, V, chunk_cap=cap, records=records or None, links=False, run_words=False)
        exact = built.compact(hip.lib)
        for plan, x, G, lo in zip((staged, built, exact), tabs, Gs, losses):
            hip.step_sparse(plan, x, h, G, lo)
        assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2]), (k, [lo.tolist() for lo in losses])
        if name == "heavy":
            assert exact.host_counts[4] > 0 and exact.host_counts[4] < staged.cap_heavy     # empty heavy blocks ran
        ref.train_step(t, *(a.cpu().numpy() for a in arrays), hp)
    for other in tabs[1:]:
        for n_ in ("R", "C", "br", "bc"):
            assert torch.equal(getattr(tabs[0], n_), getattr(other, n_)), n_
            assert torch.equal(tabs[0].s1[n_], other.s1[n_]), "slot1 " + n_
            if n_ in tabs[0].s2:
                assert torch.equal(tabs[0].s2[n_], other.s2[n_]), "slot2 " + n_
        assert torch.equal(tabs[0].scalars, other.scalars) and tabs[0].global_step == other.global_step
    assert_opt_tables_close(tabs[0], t, *TRAJ_TOL)
    for G in Gs:
        _assert_buffer_zero(G)


# ---- F: touched-rows exchange on one GPU --------------------------------------------------------------------------------
ROWS_CONFIGS = [c for c, i in zip(CONFIGS, CONFIG_IDS) if i in ("SGD", "SGD-momentum", "Adamax", "Adadelta", "Ftrl", "Nadam")]
ROWS_SHAPES = [s[:4] for s in SHAPES if s[2] in (1, 100, 150, 301, 500, 700, 1024)] + [(30000, 40, 64, 8)]


@gpu
@pytest.mark.parametrize("B,V,d,cap", ROWS_SHAPES, ids=["d%d-B%d-V%d" % (s[2], s[0], s[1]) for s in ROWS_SHAPES])
@pytest.mark.parametrize("optimizer,kw,lr", ROWS_CONFIGS, ids=["SGD", "SGD-momentum", "Adamax", "Adadelta", "Ftrl", "Nadam"])
def test_f_touched_rows_exchange(hip, optimizer, kw, lr, B, V, d, cap):
    """Stepper(exchange="rows") on one rank (pack -> copy -> combine -> apply_packed_kernel) against glove_step_sparse_f32 on
    the same plan and against the oracle, three steps: bit for bit where the packing passes sum every id chunk by chunk like
    the plain passes (no chunk records, or one chunk per id), within rtol 2e-5 elsewhere; the marks come back all zero."""
    from trainer.hip_api import DeviceTables
    from trainer.stepper import HipBackend, Stepper
    if V == 40:
        row, col, w, y = _heavy_batch(B, V)
    else:
        row, col, w, y = make_batch(77 + d, B, V)
    hp, _ = _hyper(optimizer, kw, lr, B)
    t = oracle_tables(V, d, optimizer)
    tabs = [opt_tables_from_oracle(t, DeviceTables) for _ in range(2)]
    backend = HipBackend("cuda:0")
    plan = hip.build_plan(*to_dev(row, col, w, y), V, chunk_cap=cap, compact=True)
    kw_ = dict(l2_reg=hp.l2_reg, reg_mult=hp.reg_mult, learning_rate=lr, optimizer=optimizer, **kw)
    rows, plain = Stepper(backend, tabs[0], kw_, B, exchange="rows"), Stepper(backend, tabs[1], kw_, B)
    rows.prepare([plan])
    plain.prepare([plan])
    assert rows.rows and [n for n, _ in rows.phases()] == ["passes", "pack_grad", "all_gather", "combine_apply"]
    assert [n for n, _ in plain.phases()] == ["step"]
    rows.G.fill_(float("nan"))                        # whatever the buffer holds: first touches store, they do not add
    for _ in range(3):
        rows.step(plan)
        plain.step(plan)
        want = ref.train_step(t, row, col, w, y, hp)
        assert int(rows.bufs["mark"].abs().max()) == 0
    if plan.r_crec is None or plan.host_counts[6] == 1:
        for n in ("R", "C", "br", "bc"):
            assert torch.equal(getattr(tabs[0], n), getattr(tabs[1], n)), n
            assert torch.equal(tabs[0].s1[n], tabs[1].s1[n]), "slot1 " + n
            if n in tabs[0].s2:
                assert torch.equal(tabs[0].s2[n], tabs[1].s2[n]), "slot2 " + n
        assert torch.equal(tabs[0].scalars, tabs[1].scalars)
        assert torch.equal(rows.loss_out[:3], plain.loss_out[:3]), (rows.loss_out.view(torch.int32).tolist(),
                                                                    plain.loss_out.view(torch.int32).tolist())
    else:
        for n in ("R", "C", "br", "bc"):
            torch.testing.assert_close(getattr(tabs[0], n), getattr(tabs[1], n), rtol=2e-5, atol=2e-6)
            torch.testing.assert_close(tabs[0].s1[n], tabs[1].s1[n], rtol=2e-5, atol=2e-6)
            if n in tabs[0].s2:
                torch.testing.assert_close(tabs[0].s2[n], tabs[1].s2[n], rtol=2e-5, atol=2e-6)
        torch.testing.assert_close(rows.loss_out[:3], plain.loss_out[:3], rtol=2e-5, atol=0)
    np.testing.assert_allclose(rows.loss_out.cpu().numpy()[:3], want, rtol=LOSS_RTOL)
    for x in tabs:
        assert_opt_tables_close(x, t, *TRAJ_TOL)
    _assert_buffer_zero(plain._rms_G)


# ---- G: the tagged (one-launch) form on a dealt batch that holds a heavy id ---------------------------------------------
@gpu
@pytest.mark.parametrize("optimizer", ["Adagrad", "Adam"])
def test_g_tagged_form_on_a_dealt_heavy_batch(hip, optimizer):
    """AUTO takes the one-launch form for a staging plan of at most 2,048 pairs on tagged tables — its host counts are
    unknown, so a heavy id does not keep it away.  That form sums the chunks of a heavy id in its own order: the result is
    close to the oracle, bitwise repeatable, and bit for bit the forced GLOVE_STEP_TAGGED on glove_plan_build of the same batches."""
    from trainer.hip_api import STEP_TAGGED, DeviceTables, Pairs, PlanBlock, make_hyper
    from helpers import assert_tables_close, tables_from_oracle
    B, V, d, cap = 2048, 3000, 64, 32
    n = 3 * B + 77
    row, col, w, y = make_batch(31, n, V)
    row[np.random.default_rng(6).random(n) < 0.3] = 5            # ~600 pairs of every batch: > 8 chunks of 32
    col[row == col] = (col[row == col] + 1) % V
    m = hip.build_masters(*to_dev(row, col, w, y), V)
    rs, cs = Pairs(n, "cuda:0"), Pairs(n, "cuda:0")
    hip.deal_epoch(m, B, KEY, rs, cs, hip.deal_workspace(n, B, "cuda:0"))
    nb = n // B
    block = PlanBlock([hip.staging_plan(B, V, cap, "cuda:0", records=True) for _ in range(nb)])
    ws = torch.empty(hip.lib.glove_plan_sorted_workspace_bytes(B, nb), dtype=torch.uint8, device="cuda:0")
    hip.build_plans_sorted(rs, cs, 0, block, nb, V, ws)
    lr = 0.05 if optimizer == "Adagrad" else 0.001
    hp = ref.Hyper(learning_rate=lr)
    t = oracle_tables(V, d, optimizer)
    auto = make_hyper(l2_reg=hp.l2_reg, reg_mult=hp.reg_mult, learning_rate=lr, batch_size=B)
    forced = make_hyper(l2_reg=hp.l2_reg, reg_mult=hp.reg_mult, learning_rate=lr, batch_size=B, step_form=STEP_TAGGED)
    runs = []
    for arm in ("staged", "staged", "built"):
        dt = tables_from_oracle(t, DeviceTables)
        dt.maybe_enable_tags(B)
        assert dt.R_tag is not None
        G = hip.dense_grad_buffer(dt) if optimizer == "Adam" else None
        loss_out = torch.zeros(4, device="cuda:0")
        losses = []
        for k in range(nb):
            if arm == "staged":
                plan, h = block.plans[k], auto
                assert plan.host_counts[4] < 0 and plan.r_crec is not None and plan.r_mark is not None
                assert int(plan.counts[4]) > 0, "the dealt batch holds no heavy id"
            else:
                plan, h = hip.build_plan(*(a.contiguous() for a in rs.arrays(k * B, (k + 1) * B)), V, chunk_cap=cap, records=True), forced
            if optimizer == "Adagrad":
                hip.step_adagrad(plan, dt, h, loss_out)
            else:
                hip.step_adam(plan, dt, h, G, loss_out)
            losses.append(loss_out.clone())
        runs.append((dt, losses))
    t1 = t.copy()
    for k in range(nb):
        want = ref.train_step(t1, *(a.cpu().numpy() for a in rs.arrays(k * B, (k + 1) * B)), hp)
        np.testing.assert_allclose(runs[0][1][k].cpu().numpy()[:3], want, rtol=LOSS_RTOL)
    assert_tables_close(runs[0][0], t1, *TRAJ_TOL)
    for dt, losses in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], losses))
        for n_ in ("R", "C", "br", "bc"):
            assert torch.equal(getattr(runs[0][0], n_), getattr(dt, n_)), n_
            assert torch.equal(runs[0][0].s1[n_], dt.s1[n_]), "slot1 " + n_
            if n_ in dt.s2:
                assert torch.equal(runs[0][0].s2[n_], dt.s2[n_]), "slot2 " + n_
        assert torch.equal(runs[0][0].scalars[:3], dt.scalars[:3]) and runs[0][0].global_step == dt.global_step


# ---- H: the one dispatch against the per-name wrappers -----------------------------------------------------------------
DISPATCH_NAMES = ["Adagrad", "SGD", "RMSprop", "Adamax", "Adam", "Adadelta", "Ftrl", "Nadam", "LazyAdam", "RowWiseAdagrad"]


def _quarter_on_id_0(seed, B, V):
    """A batch whose id 0 holds a quarter of the pairs on both sides (every fourth row, every fourth col) and ten more."""
    row, col, w, y = make_batch(seed, B, V, zipf=False)
    row, col = 1 + row % (V - 1), 1 + col % (V - 1)
    clash = row == col
    col[clash] = col[clash] % (V - 1) + 1
    row[0::4], row[2:40:4] = 0, 0
    col[1::4], col[3:40:4] = 0, 0
    return row, col, w, y


@gpu
@pytest.mark.parametrize("optimizer", DISPATCH_NAMES)
def test_h_step_dispatch_equals_the_names_own_wrapper(hip, optimizer):
    """GloveHip.step picks the entry point from tables.optimizer; step_adagrad / step_adam / step_sparse are the wrappers it
    stands for.  Three steps through each from the same seed, d = 50 on a stride of 52 (padding columns), chunks of 8 with an id
    of more than 8 chunks on both sides (the workgroup path): both reach the same launches, so all four variables, every
    slot, scalars, global_step and the loss are bitwise equal.  No tolerance."""
    from trainer.hip_api import DeviceTables, make_hyper
    V, d, B, cap = 97, 50, 256, 8
    batches = [_quarter_on_id_0(900 + s, B, V) for s in range(3)]
    for row, col, _, _ in batches:
        assert int((row == 0).sum()) == int((col == 0).sum()) == B // 4 + 10 > 8 * cap and not (row == col).any()     # id 0: more than HEAVY_CHUNKS chunks
    plans = [hip.build_plan(*to_dev(*b), V, chunk_cap=cap) for b in batches]
    h = make_hyper(learning_rate=0.01, batch_size=B, optimizer=optimizer)
    runs = []
    for arm in ("dispatch", "wrapper"):
        dt = DeviceTables(V, d, optimizer, seed=3)
        assert dt.d == 52
        G = hip.dense_grad_buffer(dt) if optimizer in ("Adam", "RMSprop", "Nadam") else None
        loss_out = torch.zeros(4, device="cuda:0")
        for plan in plans:
            if arm == "dispatch":
                hip.step(plan, dt, h, G, loss_out)
            elif optimizer == "Adagrad":
                hip.step_adagrad(plan, dt, h, loss_out)
            elif optimizer == "Adam":
                hip.step_adam(plan, dt, h, G, loss_out)
            else:
                hip.step_sparse(plan, dt, h, G, loss_out)
        _assert_buffer_zero(G)
        runs.append((dt, loss_out))
    (a, la), (b, lb) = runs
    assert a.global_step == b.global_step == 3
    for n in ("R", "C", "br", "bc"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
        assert torch.equal(a.s1[n], b.s1[n]), "slot1 " + n
        assert set(a.s2) == set(b.s2)
        if n in a.s2:
            assert torch.equal(a.s2[n], b.s2[n]), "slot2 " + n
    assert torch.equal(a.scalars, b.scalars) and torch.equal(la, lb)
    assert float(a.R.abs().max()) > 0 and not torch.equal(a.R, DeviceTables(V, d, optimizer, seed=3).R)       # the steps moved something
