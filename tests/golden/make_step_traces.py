"""Generates tests/golden/step_call_traces.json: which C entry points a step of every optimizer name reaches from the
host code (trainer.stepper, trainer.hip_api), and with which of the arguments that the host code decides.

    python tests/golden/make_step_traces.py         # rewrites tests/golden/step_call_traces.json

The trace is pure host logic and runs without a GPU: DeviceTables and Plans live on the CPU (the plans' host counts filled
in by hand), `hip_api._stream` returns 0, the `_require` checks for device tensors are off, and the loaded library is replaced
by a recorder that returns 0 from every compute entry point and hands the pure host size queries (`*_bytes`,
glove_dense_grad_layout, glove_plan_chunk_bound) to the real libglove_hip.so.  tests/test_step_dispatch.py runs the same
code and asserts equality with the committed file: the file pins the dispatch, it is regenerated only when the dispatch is
meant to change.

Recorded per call: the entry point; hyper.sides; hyper.optimizer for the entry points include/glove_hip.h says read it;
whether G_flat / loss_out are null (for the entry points that take them); the number of plans (the chained entry points);
whether the tables struct carries R_tag / R_ver."""
import contextlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
OUT = HERE / "step_call_traces.json"

V, D, B, CAP = 24, 8, 16, 8
NAMES = ("Adagrad", "SGD", "RMSprop", "Adamax", "Adam", "Adadelta", "Ftrl", "Nadam", "LazyAdam", "RowWiseAdagrad")
LISTS_ONLY = ("SGD", "Adamax", "Adadelta", "Ftrl", "Nadam", "LazyAdam", "RowWiseAdagrad")     # no dense exchange on several ranks
READS_OPTIMIZER = ("glove_dense_adam_f32", "glove_apply_packed_adagrad_f32", "glove_rowside_step_f32", "glove_step_sparse_f32")
# positions of (G_flat, loss_out) in the argument lists (include/glove_hip.h); None: the entry point has no such argument
G_AND_LOSS = {
    "glove_step_adagrad_f32": (None, 5), "glove_steps_adagrad_f32": (None, 6),
    "glove_step_adam_f32": (5, 6), "glove_steps_adam_f32": (6, 7), "glove_step_sparse_f32": (5, 6),
    "glove_apply_adagrad_f32": (None, 5), "glove_dense_grad_f32": (5, None),
    "glove_dense_adagrad_f32": (2, 3), "glove_dense_adam_f32": (2, 3), "glove_rowside_step_f32": (5, None),
    "glove_count_packed_f32": (3, None), "glove_combine_packed_f32": (3, None), "glove_apply_packed_adagrad_f32": (4, 7),
}
HOST_QUERIES = ("glove_abi_version", "glove_dense_grad_layout", "glove_plan_chunk_bound")


class Recorder:
    """Stands in for the loaded library."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_bytes") or name in HOST_QUERIES:
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append(self.describe(name, args))
            return 0
        return entry

    @staticmethod
    def describe(name, args):
        from trainer.hip_api import GloveHyper, GlovePlan, GloveTables
        call = {"fn": name}
        for i, a in enumerate(args):
            obj = getattr(a, "_obj", None)              # what C.byref() points at
            if isinstance(obj, GloveHyper):
                call["sides"] = obj.sides
                if name in READS_OPTIMIZER:
                    call["optimizer"] = obj.optimizer
            elif isinstance(obj, GloveTables):
                call["R_tag"], call["R_ver"] = obj.R_tag is not None, obj.R_ver is not None
            elif isinstance(obj, GlovePlan):
                call["plans"] = 1
            elif i == 0 and name.startswith("glove_steps_"):
                call["plans"] = int(args[1])
        g, loss = G_AND_LOSS.get(name, (None, None))
        if g is not None:
            call["G_null"] = args[g] is None
        if loss is not None:
            call["loss_null"] = args[loss] is None
        return call


class StubDist:
    """A torch.distributed whose collectives do nothing (one rank: the buffers already hold what they would deliver)."""

    class ReduceOp:
        MAX, MIN = "max", "min"

    class Work:
        def wait(self):
            pass

    def get_backend(self):
        return "stub"

    def all_reduce(self, t, op=None, async_op=False):
        return self.Work()

    def all_gather_into_tensor(self, out, inp, async_op=False):
        return self.Work()


@contextlib.contextmanager
def recording():
    sys.path[:0] = [p for p in (str(REPO),) if p not in sys.path]
    from trainer import hip_api
    saved = hip_api._lib, hip_api._stream, hip_api._require
    rec = Recorder(hip_api.load_library())
    hip_api._lib, hip_api._stream, hip_api._require = rec, (lambda: 0), (lambda *a, **k: None)
    try:
        yield rec
    finally:
        hip_api._lib, hip_api._stream, hip_api._require = saved


def make_plan():
    from trainer.hip_api import Plan
    plan = Plan(B, V, CAP, "cpu")
    plan.host_counts = [14, 12, 13, 11, 0, -1, 2, -1]       # chunks / ids of the row side, of the col side, heavy ids, -, most chunks of an id, -
    return plan


def build_traces() -> dict:
    import torch
    with recording() as rec:
        from trainer.hip_api import DeviceTables, make_hyper
        from trainer.stepper import HipBackend, RowShardedStepper, Stepper
        cases = {}

        def take():
            calls, rec.calls = rec.calls, []
            return calls

        def tables(name):
            return DeviceTables(V, D, name, device="cpu", seed=0)

        for name in NAMES:
            kw = dict(learning_rate=0.05, optimizer=name, step_form=0)
            plans = [make_plan() for _ in range(3)]

            # Stepper on one rank: a step, three steps at once, a step again (what a chained call left is brought home)
            t = tables(name)
            st = Stepper(HipBackend("cpu"), t, kw, B)
            take()
            if name in ("Adagrad", "Adam"):                 # maybe_enable_tags has fired: B <= 2048, 2 B <= 2 V
                assert t.R_tag is not None
            case = {"tagged": t.R_tag is not None, "twinned": t.R_ver is not None, "dense": bool(st.dense)}
            st.step(plans[0])
            case["step"] = take()
            st.step_many(plans)
            case["step_many"] = take()
            st.step(plans[0])
            case["step_again"] = take()
            _ = t.R                                         # a reader of the row table: brings a tagged table home first
            case["read_R"] = take()
            cases["Stepper/%s" % name] = case

            # RowShardedStepper alone in the world: the plain step
            t = tables(name)
            st = RowShardedStepper(HipBackend("cpu"), t, kw, B, 1, None)
            take()
            st.step(plans[0])
            cases["RowShardedStepper/world1/%s" % name] = {"tagged": t.R_tag is not None, "G": st.G is not None, "step": take()}

            # ... and through the transport, in the exchanges the name may take
            for exchange in (("rows",) if name in LISTS_ONLY else ("dense", "rows")):
                t = tables(name)
                st = RowShardedStepper(HipBackend("cpu"), t, kw, B, 1, StubDist(), exchange=exchange, collectives=True)
                st.prepare([plans[0]])
                take()
                st.step(plans[0])
                cases["RowShardedStepper/collectives/%s/%s" % (exchange, name)] = {"rows": bool(st.rows), "step": take()}

            # HipBackend.rowside_step without a buffer lent: the scratch it keeps
            t = tables(name)
            b = HipBackend("cpu")
            b.rowside_step(plans[0], t, make_hyper(batch_size=B, sides=1, **kw))
            cases["rowside_step/%s" % name] = {"calls": take(), "scratch": sorted(list(g.shape) for g in b._row_G.values())}

            # HipBackend.apply_dense
            t = tables(name)
            b = HipBackend("cpu")
            try:
                b.apply_dense(t, make_hyper(batch_size=B, **kw), b.dense_grad_buffer(t), torch.zeros(4))
                cases["apply_dense/%s" % name] = {"calls": take()}
            except ValueError as exc:
                cases["apply_dense/%s" % name] = {"calls": take(), "error": "ValueError: %s" % exc}
    return {"shape": {"V": V, "d": D, "B": B, "chunk_cap": CAP}, "cases": cases}


def main():
    OUT.write_text(json.dumps(build_traces(), indent=1, sort_keys=True) + "\n")
    print("written", OUT)


if __name__ == "__main__":
    main()
