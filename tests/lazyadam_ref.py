"""TEST-ONLY float64 restatement of LazyAdam (include/glove_hip.h GLOVE_OPT_LAZYADAM): Adam that moves only the rows a batch
touches.  The forward pass and the summed gradients are the oracle's own (oracle/glove_ref.py `gradients`: activity-L2 term
included, duplicates summed); only the update is stated here:

    t    = global_step + 1                      (the GLOBAL step, also for a row last touched long ago)
    lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)
    for every distinct id of the batch, on each side:   m = beta1 m + (1 - beta1) G
                                                        v = beta2 v + (1 - beta2) G^2
                                                        var -= lr_t m / (sqrt(v) + epsilon)
    every other row keeps var, m and v; the global bias (a dense variable) takes the same update every step.

The tables are the oracle's Adam tables (slots M_*, V_*, zeros) under the name "LazyAdam".  Never imported by the product."""
import math

import numpy as np
import torch

import glove_ref as ref
import helpers

OPTIMIZER = "LazyAdam"
# the device slots s1, s2 of LazyAdam are the oracle's M_ and V_, like Adam's and Adamax's: lets helpers.opt_tables_from_oracle
# and helpers.assert_opt_tables_close (padding columns, scalars, global_step) serve the ninth name as they serve the eight
helpers.SLOTS.setdefault(OPTIMIZER, ("M_", "V_"))


def tables(V, d, dtype=np.float64, seed=1):
    """float64 tables whose values are exactly representable in fp32 (as helpers.oracle_tables), m and v zeros."""
    t = ref.Tables(V, d, "Adam", dtype=np.float32, seed=seed)
    t.optimizer = OPTIMIZER
    return t.astype(dtype)


def lr_t(hp, step_after, dt=np.float64):
    """The bias-corrected step size of the step that ends with global_step == step_after, hyper-parameters cast to fp32 first as
    Keras casts them to the variable dtype (and as oracle/glove_ref.py does for Adam)."""
    lr, b1, b2 = (float(np.float32(x)) for x in (hp.learning_rate, hp.beta1, hp.beta2))
    return dt(lr * math.sqrt(1.0 - b2 ** step_after) / (1.0 - b1 ** step_after))


def _rows(W, M, Vv, G, touched, lt, b1, b2, eps):
    """The touched rows only, in place; nothing else is read or written."""
    g = G[touched]
    M[touched] = b1 * M[touched] + (1 - b1) * g
    Vv[touched] = b2 * Vv[touched] + (1 - b2) * g * g
    W[touched] -= lt * M[touched] / (np.sqrt(Vv[touched]) + eps)


def apply_update(t, gr, hp, sides=3, base=None):
    """The LazyAdam update from summed gradients `gr` on the sides `sides` selects (1 row side, 2 col side, 3 both); the scalar
    work (global bias with its moments, global_step) goes with the col side.  base: the tables whose global bias and
    global_step a view of them stands for (a sharded form's view of fetched col rows)."""
    base = t if base is None else base
    dt = t.dtype
    eps = dt(np.float32(hp.epsilon))
    b1, b2 = dt(np.float32(hp.beta1)), dt(np.float32(hp.beta2))
    lt = lr_t(hp, base.step + 1, dt)
    if sides & 1:
        _rows(t.R, t.M_R, t.V_R, gr["G_R"], gr["touched_r"], lt, b1, b2, eps)
        _rows(t.br, t.M_br, t.V_br, gr["G_br"], gr["touched_r"], lt, b1, b2, eps)
    if sides & 2:
        _rows(t.C, t.M_C, t.V_C, gr["G_C"], gr["touched_c"], lt, b1, b2, eps)
        _rows(t.bc, t.M_bc, t.V_bc, gr["G_bc"], gr["touched_c"], lt, b1, b2, eps)
        dg = gr["sum_e"] + gr.get("dg_reg", 2.0 * hp.reg_mult * hp.l2_reg * base.g)
        base.M_g = b1 * base.M_g + (1 - b1) * dg
        base.V_g = b2 * base.V_g + (1 - b2) * dg * dg
        base.g = base.g - lt * base.M_g / (np.sqrt(base.V_g) + eps)
        base.step += 1


def train_step(t, row, col, w, y, hp):
    """One step on one batch.  Returns (loss, L, Reg) as glove_ref.train_step does."""
    gr = ref.gradients(t, row, col, w, y, hp)
    reg = gr["reg"] + gr["reg_g"]
    loss = gr["L"] + t.dtype(hp.reg_mult) * reg
    apply_update(t, gr, hp)
    return loss, gr["L"], reg


def device_tables(t, DeviceTables, device="cuda:0"):
    """Device tables holding exactly the (fp32-rounded) state of `t`."""
    return helpers.opt_tables_from_oracle(t, DeviceTables, device)


def snapshot(dt):
    """Clones of every variable, both slots and the scalars of device tables (for bit-for-bit comparisons)."""
    out = {"scalars": dt.scalars.clone(), "step": dt.step.clone()}
    for n in ("R", "C", "br", "bc"):
        out[n], out["m_" + n], out["v_" + n] = getattr(dt, n).clone(), dt.s1[n].clone(), dt.s2[n].clone()
    return out


def assert_bitwise_equal(a, b, what=""):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s %s differs" % (what, k)
