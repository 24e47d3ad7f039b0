"""TEST CASE run in a process of its own by tests/test_gpu_sharded_optimizers.py (an RCCL process group of its own, as
tests/rccl_graph_case.py says why): the sharded forms under the dense-decay optimizers, a step captured once as a hipGraph —
kernels, the row side's scratch, the owner's apply with its own hyper, the RCCL collectives — and replayed == the same steps
launched eagerly, bit for bit."""
import faulthandler
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for _p in (REPO, REPO / "oracle", REPO / "tests"):
    sys.path.insert(0, str(_p))
import numpy as np      # noqa: E402
import torch            # noqa: E402
import glove_ref as ref  # noqa: E402


def run(hip):
    import os
    import torch.distributed as dist
    from helpers import make_batch, opt_tables_from_oracle, to_dev
    from trainer.hip_api import DeviceTables
    from trainer.stepper import HipBackend, RowShardedStepper, ShardedStepper
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("CASE_PORT", "29553"), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", device_id=torch.device("cuda:0"))
    try:
        B, V, d, nb, rounds = 6000, 700, 64, 3, 4
        backend = HipBackend("cuda:0")
        batches = [to_dev(*make_batch(70 + s, B, V)) for s in range(nb)]
        plans = [backend.build_plan(*bt, V, 0).compact(hip.lib, d) for bt in batches]
        for opt in ("Adam", "RMSprop", "Nadam"):
            t = ref.Tables(V, d, opt, dtype=np.float32, seed=4).astype(np.float64)
            kw = dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.01, optimizer=opt)

            def make(form):
                tabs = opt_tables_from_oracle(t, DeviceTables)
                if form.startswith("row-sharded"):
                    st = RowShardedStepper(backend, tabs, kw, B, 1, dist, exchange=form.split()[1], collectives=True)
                    st.prepare(plans)
                    return tabs, st, plans
                st = ShardedStepper(backend, tabs, kw, B, 1, 0, dist, collectives=True, exercise_exchange=True)
                return tabs, st, [st.add_batch(*bt) for bt in batches]
            forms = ("row-sharded rows", "both tables sharded") + (("row-sharded dense",) if opt != "Nadam" else ())
            for form in forms:
                (ta, sa, ia), (tb, sb, ib) = make(form), make(form)
                sb.enable_graphs(after=1)
                assert sb._graphs is not None, form
                for rnd in range(rounds):
                    for k in range(nb):
                        sa.step(ia[k])
                        sb.step(ib[k])                      # round 0 eager, round 1 captures and replays, then replays
                    if rnd == 1:
                        assert len(sb._graphs) == nb, (opt, form)
                for n in ("R", "C", "br", "bc"):
                    assert torch.equal(getattr(ta, n), getattr(tb, n)), (opt, form, n)
                    for slots_a, slots_b in ((ta.s1, tb.s1), (ta.s2, tb.s2)):
                        if n in slots_a:
                            assert torch.equal(slots_a[n], slots_b[n]), (opt, form, n)
                # (Nadam: the momentum cache slot no step has written yet holds NaN in both: compare the bits)
                assert torch.equal(ta.scalars.view(torch.int32), tb.scalars.view(torch.int32)), (opt, form)
                assert ta.global_step == tb.global_step == rounds * nb, (opt, form)
                assert torch.equal(sa.loss_out, sb.loss_out), (opt, form)
                sb.release_graphs()
    finally:
        import gc
        for obj in gc.get_objects():
            if isinstance(obj, (RowShardedStepper, ShardedStepper)):
                obj.release_graphs()
        gc.collect()
        dist.destroy_process_group()


if __name__ == "__main__":
    faulthandler.dump_traceback_later(200, exit=True)
    from trainer.hip_api import GloveHip
    run(GloveHip("cuda:0"))
    print("sharded graph case ok", flush=True)
