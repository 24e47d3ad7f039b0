"""TEST-ONLY float64 restatement of RowWiseAdagrad (include/glove_hip.h GLOVE_OPT_ROWWISE_ADAGRAD): Adagrad with ONE accumulator
per embedding row, as FBGEMM / TorchRec apply it to embedding tables.  The forward pass and the summed gradients are the
oracle's own (oracle/glove_ref.py `gradients`: activity-L2 term included, duplicates summed); only the update is stated here:

    for every distinct id u of the batch, on each side:   A[u]    += mean_j G[u, j]^2          (over the d real columns)
                                                          W[u, :] -= lr G[u, :] / (sqrt(A[u]) + epsilon)     (A[u] as incremented)
    br, bc (one float per row anyway) and the global bias (a dense variable, every step) take plain Keras Adagrad;
    every other row keeps W and A.

The tables are the oracle's Adagrad tables under the name "RowWiseAdagrad" with A_R, A_C cut to float[V] (0.1).  The slot of an
embedding table is not shaped like the table, so this module carries its own device transfer, snapshot and closeness check
(tests/helpers.py assumes slot shape == variable shape in its padding checks).  Never imported by the product."""
import numpy as np
import torch

import glove_ref as ref

OPTIMIZER = "RowWiseAdagrad"
NAMES = ("R", "C", "br", "bc")


def tables(V, d, dtype=np.float64, seed=1):
    """float64 tables whose values are exactly representable in fp32 (as helpers.oracle_tables); accumulators 0.1, one per row."""
    t = ref.Tables(V, d, "Adagrad", dtype=np.float32, seed=seed)
    t.optimizer = OPTIMIZER
    t.A_R, t.A_C = t.A_R[:, 0].copy(), t.A_C[:, 0].copy()
    return t.astype(dtype)


def _rows(W, A, G, touched, lr, eps):
    """The touched embedding rows only, in place; nothing else is read or written."""
    g = G[touched]
    A[touched] += (g * g).sum(1) / W.dtype.type(W.shape[1])
    W[touched] -= lr * g / (np.sqrt(A[touched]) + eps)[:, None]


def apply_update(t, gr, hp, sides=3, base=None):
    """The update from summed gradients `gr` on the sides `sides` selects (1 row side, 2 col side, 3 both); the scalar work
    (global bias with its accumulator, global_step) goes with the col side.  base: the tables whose global bias and global_step
    a view of them stands for (a sharded form's view of fetched col rows)."""
    base = t if base is None else base
    dt = t.dtype
    lr, eps = dt(np.float32(hp.learning_rate)), dt(np.float32(hp.epsilon))        # cast to the variable dtype, as ref.apply_update
    if sides & 1:
        _rows(t.R, t.A_R, gr["G_R"], gr["touched_r"], lr, eps)
        ref._adagrad(t.br, t.A_br, gr["G_br"], gr["touched_r"], lr, eps)
    if sides & 2:
        _rows(t.C, t.A_C, gr["G_C"], gr["touched_c"], lr, eps)
        ref._adagrad(t.bc, t.A_bc, gr["G_bc"], gr["touched_c"], lr, eps)
        dg = gr["sum_e"] + gr.get("dg_reg", 2.0 * hp.reg_mult * hp.l2_reg * base.g)
        base.A_g = base.A_g + dg * dg
        base.g = base.g - lr * dg / (np.sqrt(base.A_g) + eps)
        base.step += 1


def train_step(t, row, col, w, y, hp):
    """One step on one batch.  Returns (loss, L, Reg) as glove_ref.train_step does."""
    gr = ref.gradients(t, row, col, w, y, hp)
    reg = gr["reg"] + gr["reg_g"]
    loss = gr["L"] + t.dtype(hp.reg_mult) * reg
    apply_update(t, gr, hp)
    return loss, gr["L"], reg


def device_tables(t, DeviceTables, device="cuda:0"):
    """Device tables holding exactly the (fp32-rounded) state of `t`: variables, the four accumulators (A_R, A_C one float per
    row), the global bias with its accumulator, global_step."""
    dt = DeviceTables(t.V, t.d, OPTIMIZER, device=device, seed=0)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(device)
    dm = dt.d_model
    for n in NAMES:
        x = getattr(dt, n)
        (x[:, :dm] if x.dim() == 2 else x).copy_(f(getattr(t, n)))
        assert dt.s1[n].shape == (x.shape[0],), "slot 1 of %s is %s" % (n, tuple(dt.s1[n].shape))
        dt.s1[n].copy_(f(getattr(t, "A_" + n)))
    sc = np.zeros(8, np.float32)
    sc[0], sc[1] = t.g, t.A_g
    dt.scalars.copy_(torch.from_numpy(sc))
    dt.step.fill_(t.step)
    return dt


def snapshot(dt):
    """Clones of every variable, every accumulator and the scalars of device tables (for bit-for-bit comparisons)."""
    out = {"scalars": dt.scalars.clone(), "step": dt.step.clone()}
    for n in NAMES:
        out[n], out["a_" + n] = getattr(dt, n).clone(), dt.s1[n].clone()
    return out


def assert_bitwise_equal(a, b, what=""):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s %s differs" % (what, k)


def _close(got, want, rtol, atol, what):
    w = torch.from_numpy(np.ascontiguousarray(want, np.float64)).to(got.device)
    ok = (got.double() - w).abs() <= atol + rtol * w.abs()          # (NaN never passes)
    if not bool(ok.all()):
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=rtol, atol=atol, err_msg=what)
        raise AssertionError("%s: %d entries outside rtol %g / atol %g" % (what, int((~ok).sum()), rtol, atol))


def assert_tables_close(dt, t, rtol=1e-5, atol=1e-6):
    """Every variable and accumulator against the restatement; the padding columns of R and C exactly zero; slot 1 one float
    per row on all four variables, no slot 2; the global bias and its accumulator; global_step."""
    dm = dt.d_model
    assert not dt.s2, "RowWiseAdagrad keeps no second slot"
    for n in NAMES:
        x = getattr(dt, n)
        _close(x[:, :dm] if x.dim() == 2 else x, getattr(t, n), rtol, atol, n)
        if x.dim() == 2 and dt.d > dm:
            assert float(x[:, dm:].abs().max()) == 0.0, n + " padding moved"
        assert dt.s1[n].dim() == 1 and dt.s1[n].shape[0] == x.shape[0], "slot 1 of " + n
        _close(dt.s1[n], getattr(t, "A_" + n), rtol, atol, "A_" + n)
    sc = dt.scalars.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(sc[0], t.g, rtol=rtol, atol=atol, err_msg="global_bias")
    np.testing.assert_allclose(sc[1], t.A_g, rtol=rtol, atol=atol, err_msg="A_g")
    assert dt.global_step == t.step
