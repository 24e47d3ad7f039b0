"""TEST-ONLY kernel provider for RowWiseAdagrad on the multi-rank forms: tests/sharded_oracle_backend.py with every apply that
would reach glove_ref.apply_update (which knows the eight Keras names only) going to tests/rowwise_adagrad_ref.py instead.
RowWiseAdagrad rides the touched-rows exchange alone, so there is no dense apply here.  Never imported by the product."""
import numpy as np

import rowwise_adagrad_ref as rw
from sharded_oracle_backend import ShardedOracleBackend


class RowWiseOracleBackend(ShardedOracleBackend):
    def step(self, plan, tables, hyper, G, loss_out):
        loss_out[0], loss_out[1], loss_out[2] = rw.train_step(tables.t, *plan, hyper["hp"])

    def rowside_step(self, plan, tables, hyper, G=None):
        assert hyper["sides"] == 1                  # (G, the scratch the steppers lend the dense-decay names, is never touched)
        base = tables._base.t if getattr(tables, "_base", None) is not None else tables.t
        rw.apply_update(tables.t, self._gr, hyper["hp"], 1, base)

    def apply_dense(self, tables, hyper, G, loss_out):
        raise AssertionError("RowWiseAdagrad has no dense apply")

    def _apply_lists(self, t, hp, lists, sides, tail, loss_out, inv_batch):
        d = t.d
        gr = dict(G_R=np.zeros_like(t.R), G_C=np.zeros_like(t.C), G_br=np.zeros_like(t.br), G_bc=np.zeros_like(t.bc),
                  touched_r=np.zeros(len(t.R), bool), touched_c=np.zeros(len(t.C), bool), sum_e=tail[0])
        for entries, ids, side in lists:                 # rank order: the ranks' rows of an id are added in that order
            for i, e in enumerate(entries):
                key = int(ids[i]) if ids is not None else int(e[d + 1])
                sd = side if side is not None else int(e[d + 2])
                GW, Gb, touched = ("G_R", "G_br", "touched_r") if sd == 0 else ("G_C", "G_bc", "touched_c")
                gr[GW][key] = gr[GW][key] + e[:d]
                gr[Gb][key] = gr[Gb][key] + e[d]
                gr[touched][key] = True
        if sides & 2:
            loss_out[1] = tail[1] * inv_batch
        rw.apply_update(t, gr, hp, sides)
