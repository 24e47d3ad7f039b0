"""TEST-ONLY kernel provider for the sharded forms under every Keras optimizer: the numpy oracle behind the interface of
`trainer.stepper.RowShardedStepper` / `ShardedStepper`, with the side-restricted applies the product has for all eight
names (tests/oracle_backend.py keeps them to Adagrad).  A side-restricted apply is `glove_ref.apply_update` itself, run on a
shallow copy of the tables whose other side is cut to zero rows: the same formulas, the same order, on the selected rows
only; the scalar work (global bias, its slots, Nadam's momentum cache, global_step) goes with the col side, as in the
product.  Never imported by the product."""
import copy

import numpy as np

import glove_ref as ref
from oracle_backend import OracleBackend

_SLOT_PREFIXES = ("", "A_", "M_", "V_", "U_", "Z_")
_SCALARS = ("g", "A_g", "M_g", "V_g", "U_g", "Z_g", "m_cache", "step")


def restricted_update(t, gr, hp, sides, base=None):
    """ref.apply_update on the sides `sides` selects (1 row side, 2 col side, 3 both) of `t`; the scalar work with the col
    side.  base: the tables whose global bias, momentum cache and global_step a view of them stands for (col_view)."""
    base = t if base is None else base
    u = copy.copy(t)
    g2 = dict(gr)
    for bit, names, keys in ((1, ("R", "br"), ("G_R", "G_br", "touched_r")), (2, ("C", "bc"), ("G_C", "G_bc", "touched_c"))):
        if sides & bit:
            continue
        for n in names:
            for p in _SLOT_PREFIXES:
                if isinstance(getattr(u, p + n, None), np.ndarray):
                    setattr(u, p + n, getattr(u, p + n)[:0])
        for k in keys:
            g2[k] = gr[k][:0]
    for a in _SCALARS:                       # the step this apply belongs to: t = base.step + 1, the base's momentum cache
        if hasattr(base, a):
            setattr(u, a, getattr(base, a))
    g2.setdefault("dg_reg", 2.0 * hp.reg_mult * hp.l2_reg * base.g)
    ref.apply_update(u, g2, hp)
    if sides & 2:
        for a in _SCALARS:
            if hasattr(u, a):
                setattr(base, a, getattr(u, a))


class ShardedOracleBackend(OracleBackend):
    def rowside_step(self, plan, tables, hyper, G=None):
        t, gr = tables.t, self._gr
        assert hyper["sides"] == 1
        base = tables._base.t if getattr(tables, "_base", None) is not None else t
        restricted_update(t, dict(gr, sum_e=0.0), hyper["hp"], 1, base)

    def apply_dense(self, tables, hyper, G, loss_out):
        t, hp, sides = tables.t, hyper["hp"], hyper["sides"]
        if t.optimizer == "Adagrad":
            return super().apply_dense(tables, hyper, G, loss_out)
        assert sides & 2, "the scalar work goes with the col side"
        G_R, G_br, G_C, G_bc, tail = self._views(tables, G)
        gr = dict(G_R=G_R.copy(), G_br=G_br.copy(), G_C=G_C.copy(), G_bc=G_bc.copy(), sum_e=tail[0],
                  dg_reg=2.0 * hp.reg_mult * hp.l2_reg * t.g)
        gr["touched_r"] = (gr["G_R"] != 0).any(1) | (gr["G_br"] != 0)
        gr["touched_c"] = (gr["G_C"] != 0).any(1) | (gr["G_bc"] != 0)
        loss_out[1] = tail[1] * hyper["inv_batch"]
        restricted_update(t, gr, hp, sides)
        G.zero_()

    def _apply_lists(self, t, hp, lists, sides, tail, loss_out, inv_batch):
        if t.optimizer == "Adagrad":
            return super()._apply_lists(t, hp, lists, sides, tail, loss_out, inv_batch)
        d = t.d
        gr = dict(G_R=np.zeros_like(t.R), G_C=np.zeros_like(t.C), G_br=np.zeros_like(t.br), G_bc=np.zeros_like(t.bc),
                  touched_r=np.zeros(len(t.R), bool), touched_c=np.zeros(len(t.C), bool),
                  sum_e=tail[0], dg_reg=2.0 * hp.reg_mult * hp.l2_reg * t.g)
        for entries, ids, side in lists:                 # rank order: the ranks' rows of an id are added in that order
            for i, e in enumerate(entries):
                key = int(ids[i]) if ids is not None else int(e[d + 1])
                sd = side if side is not None else int(e[d + 2])
                GW, Gb, touched = ("G_R", "G_br", "touched_r") if sd == 0 else ("G_C", "G_bc", "touched_c")
                if gr[touched][key]:
                    gr[GW][key] = gr[GW][key] + e[:d]
                    gr[Gb][key] = gr[Gb][key] + e[d]
                else:
                    gr[GW][key], gr[Gb][key], gr[touched][key] = e[:d], e[d], True
        if sides & 2:
            loss_out[1] = tail[1] * inv_batch
        restricted_update(t, gr, hp, sides)

    def owner_apply(self, tables, state, recv, ids, counts, hyper, tail, loss_out):
        if tables.t.optimizer == "Adagrad":
            return super().owner_apply(tables, state, recv, ids, counts, hyper, tail, loss_out)
        r, i, lists, off = recv.numpy(), ids.numpy(), [], 0
        for n in counts:
            lists.append((r[off:off + n], i[off:off + n], 1))
            off += n
        # the owner's col shard: its side only (the row shard was applied by the row side's step) + the scalar work
        self._apply_lists(tables.t, hyper["hp"], lists, 2, tail.numpy(), loss_out, hyper["inv_batch"])
