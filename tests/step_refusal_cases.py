"""The refusals of the step library (glove-tensorflow_amd/csrc/glove_step.hip): for every exported entry point that can refuse a
call, one fully valid base call at the smallest sizes that pass every check, and single-fault variants of it, one per
`return GLOVE_E_*` the source holds, each with the code the library answers.

A case names its edits only; the buffers come from the caller (an `Env`): host dummies in tests/test_step_refusals.py,
which runs without a GPU (there an accepted call comes back with a HIP error code > 0 from its first launch, so a variant
that reaches a launch before it is refused shows as > 0 too), device buffers of a real plan in
tests/test_gpu_step_refusals.py, which also holds every buffer against its bytes from before the call.

PARENT_LAUNCHED lists the variants that the library refused only after it had launched something until the step's host
side opened one validated call context (canonicalising a twinned table, the passes of a two-launch step whose apply launch
then found no slots, a sweep or a batch of lists ahead of a bad list): there the CPU run saw a HIP error code, and a GPU
saw the table's code behind those launches.  Since then they are refused before any launch, like all the others."""
import ctypes as C
from collections import namedtuple

from trainer.hip_api import GloveHyper, GlovePackedList, GlovePlan, GloveTables

BADARG, WORKSPACE = -1, -2
V, D, B = 10, 8, 4
CHUNK_CAP = 32            # DEFAULT_CHUNK_CAP; kChunkMax is as much
MARK_COUNT_MASK = 255     # kMarkCountMask: the most lists glove_count_packed_f32 counts
MAX_LISTS = 9             # the Env's list array: more than the eight a launch sees
ADAGRAD, SGD, RMSPROP, ADAMAX, ADAM, ADADELTA, FTRL, NADAM, LAZYADAM, ROWWISE = range(10)
TWO_LAUNCH, ONE_PASS, THREE_LAUNCH, FUSED_TWIN, TAGGED = 1, 2, 3, 4, 5

DUMMY = object()          # an edit's value: any valid non-null pointer of the Env


class Env:
    """What a caller provides: plans {'rec': GlovePlan with chunk records and pair arrays, 'pairs': one with pair arrays alone}
    (host_counts known), tables with both slots, pointers by name (ws, G_flat, loss_out, packed, mark, out4, ids, rows,
    biases, dummy), ws_bytes, the stream."""

    def __init__(self, plans, tables, ptr, ws_bytes, stream=None):
        self.plans, self.tables, self.ptr, self.ws_bytes, self.stream = plans, tables, ptr, ws_bytes, stream


def _copy(s):
    return type(s).from_buffer_copy(s)


class Call:
    """The arguments of one call, every one of them open to an edit."""

    def __init__(self, env, plan="rec"):
        self.env = env
        self.p, self.t, self.h = _copy(env.plans[plan]), _copy(env.tables), base_hyper()
        for k, v in env.ptr.items():
            setattr(self, k, v)
        self.ws_bytes, self.stream = env.ws_bytes, env.stream
        self.tail = None                     # glove_apply_packed_adagrad_f32 sums the headers itself
        self.capacity = self.entries_needed()
        self.n_lists, self.tag, self.n_plans, self.n_rows = 2, 0, 1, 3
        self.plans_null = self.plan0_null = self.lists_null = False
        self.lists = (GlovePackedList * MAX_LISTS)()
        for l in self.lists:
            l.entries, l.ids, l.header, l.n, l.side = self.packed, None, self.packed, -1, -1

    def entries_needed(self):
        sides = (self.h.sides & 3) or 3
        return 1 + (self.p.host_counts[1] if sides & 1 else 0) + (self.p.host_counts[3] if sides & 2 else 0)

    def ref(self, name):
        s = getattr(self, name)
        return None if s is None else C.byref(s)

    def plan_list(self):
        if self.plans_null:
            return None
        arr = (C.POINTER(GlovePlan) * max(self.n_plans, 1))()
        for i in range(max(self.n_plans, 1)):
            if self.p is not None and not (i == 0 and self.plan0_null):
                arr[i] = C.pointer(self.p)
        self._keep = arr
        return arr

    def list_array(self):
        return None if self.lists_null else self.lists


def base_hyper():
    h = GloveHyper()
    h.beta1, h.beta2, h.l2_reg, h.reg_mult, h.learning_rate, h.epsilon = 0.9, 0.999, 0.01, 2.0, 0.05, 1e-7
    h.inv_batch, h.neg_factor, h.rho = 1.0 / B, 1.0, 0.9
    return h


def _pth(c):
    return c.ref("p"), c.ref("t"), c.ref("h"), c.ws, c.ws_bytes


# entry point -> the argument list of a Call (the prototypes: trainer/hip_api.py load_library)
ENTRIES = {
    "glove_passes_f32": lambda c: (*_pth(c), c.stream),
    "glove_rowpass_f32": lambda c: (*_pth(c), c.stream),
    "glove_colpass_f32": lambda c: (*_pth(c), c.stream),
    "glove_apply_adagrad_f32": lambda c: (*_pth(c), c.loss_out, c.stream),
    "glove_dense_grad_f32": lambda c: (*_pth(c), c.G_flat, c.stream),
    "glove_dense_adagrad_f32": lambda c: (c.ref("t"), c.ref("h"), c.G_flat, c.loss_out, c.stream),
    "glove_dense_adam_f32": lambda c: (c.ref("t"), c.ref("h"), c.G_flat, c.loss_out, c.stream),
    "glove_pack_grad_f32": lambda c: (*_pth(c), c.packed, c.capacity, c.stream),
    "glove_passes_packing_f32": lambda c: (*_pth(c), c.packed, c.capacity, c.stream),
    "glove_pack_rest_f32": lambda c: (*_pth(c), c.packed, c.capacity, c.stream),
    "glove_loss_partials_f32": lambda c: (c.ref("p"), c.ref("t"), c.ws, c.ws_bytes, c.out4, c.stream),
    "glove_combine_packed_f32": lambda c: (c.list_array(), c.tag, c.ref("t"), c.G_flat, c.mark, c.capacity, c.stream),
    "glove_count_packed_f32": lambda c: (c.list_array(), c.n_lists, c.ref("t"), c.G_flat, c.mark, c.capacity, c.stream),
    "glove_apply_packed_adagrad_f32": lambda c: (c.list_array(), c.n_lists, c.ref("t"), c.ref("h"), c.G_flat, c.mark, c.tail,
                                                 c.loss_out, c.capacity, c.stream),
    "glove_gather_rows_f32": lambda c: (c.t.R, c.t.br, c.ids, c.n_rows, c.t.d, c.rows, c.biases, c.stream),
    "glove_canonicalize_f32": lambda c: (c.ref("t"), c.stream),
    "glove_step_adagrad_f32": lambda c: (*_pth(c), c.loss_out, c.stream),
    "glove_rowside_step_adagrad_f32": lambda c: (*_pth(c), c.stream),
    "glove_steps_adagrad_f32": lambda c: (c.plan_list(), c.n_plans, c.ref("t"), c.ref("h"), c.ws, c.ws_bytes, c.loss_out, c.stream),
    "glove_step_adam_f32": lambda c: (*_pth(c), c.G_flat, c.loss_out, c.stream),
    "glove_step_sparse_f32": lambda c: (*_pth(c), c.G_flat, c.loss_out, c.stream),
    "glove_rowside_step_f32": lambda c: (*_pth(c), c.G_flat, c.stream),
    "glove_steps_adam_f32": lambda c: (c.plan_list(), c.n_plans, c.ref("t"), c.ref("h"), c.ws, c.ws_bytes, c.G_flat, c.loss_out, c.stream),
}


def put(path, value):
    """An edit: 't.d' / 'h.head' / 'p.host_counts' name a struct's field, a bare name an argument of the call; DUMMY stands for a
    valid pointer, a callable value is called with the Call."""
    def edit(c):
        v = c.dummy if value is DUMMY else value(c) if callable(value) else value
        obj, _, field = path.rpartition(".")
        setattr(getattr(c, obj) if obj else c, field, v)
    return edit


def bad_list(i, field, value):
    return lambda c: setattr(c.lists[i], field, value)


# what an entry point's base call differs in from the common one
BASE = {
    "glove_dense_adam_f32": (put("h.optimizer", ADAM),),
    "glove_canonicalize_f32": (put("t.R_ver", DUMMY),),                  # (a plain table is done without a launch)
    "glove_rowside_step_adagrad_f32": (put("h.sides", 1),),
    "glove_rowside_step_f32": (put("h.sides", 1), put("h.optimizer", SGD)),
    "glove_step_adam_f32": (put("h.optimizer", ADAM),),
    "glove_steps_adam_f32": (put("h.optimizer", ADAM),),
    "glove_step_sparse_f32": (put("h.optimizer", SGD),),
}

Case = namedtuple("Case", "entry name edits code plan")
CASES = []


def case(entry, name, code, *edits, plan="rec"):
    CASES.append(Case(entry, name, BASE.get(entry, ()) + tuple(edits), code, plan))


def case_id(c):
    return "%s:%s%s" % (c.entry, c.name, "" if c.plan == "rec" else "@" + c.plan)


TWIN = put("t.R_ver", DUMMY)
TAGS = (put("t.R_tag", DUMMY), put("t.C_tag", DUMMY))
BIG_TWIN = put("t.V", 1 << 26)        # x d x 4 B: 2^31, twice that no 32-bit row offset


def common(entry):
    """Every clause of check_common and the workspace size, for an entry point that takes (p, t, h, ws, ws_bytes)."""
    for name in ("p", "t", "h", "ws"):
        case(entry, "null " + name, BADARG, put(name, None))
    case(entry, "B -1", BADARG, put("p.B", -1))
    case(entry, "cap_chunks -1", BADARG, put("p.cap_chunks", -1))
    case(entry, "V 0", BADARG, put("t.V", 0))
    case(entry, "V -1", BADARG, put("t.V", -1))
    for d in (0, 6, 1028):
        case(entry, "d %d" % d, BADARG, put("t.d", d))
    for f in ("p.counts", "t.R", "t.C", "t.br", "t.bc", "t.scalars", "t.step", "p.r_chunk_id", "p.r_chunk_start", "p.r_uniq_slot",
              "p.heavy", "p.r_uniq_rec", "p.c_uniq_rec", "p.c_chunk_id", "p.c_chunk_start", "p.c_uniq_slot"):
        case(entry, "null " + f, BADARG, put(f, None))
    case(entry, "heavy_chunks 0", BADARG, put("p.heavy_chunks", 0))
    for f in ("r_partner", "r_w", "r_y", "c_partner", "c_w", "c_y"):
        case(entry, "null p.%s, no records" % f, BADARG, put("p." + f, None), plan="pairs")
    case(entry, "no pairs, one side's records", BADARG, put("p.r_partner", None), put("p.c_crec", None))
    case(entry, "chunk_cap 0", BADARG, put("p.chunk_cap", 0))
    case(entry, "chunk_cap 33", BADARG, put("p.chunk_cap", CHUNK_CAP + 1))
    case(entry, "table of 2^32 bytes", BADARG, put("t.V", (1 << 32) // (4 * D)))
    case(entry, "V_row -1", BADARG, put("t.V_row", -1))
    case(entry, "V_row V + 1", BADARG, put("t.V_row", V + 1))
    case(entry, "R_ver, doubled table of 2^32 bytes", BADARG, TWIN, BIG_TWIN)
    case(entry, "R_tag without C_tag", BADARG, put("t.R_tag", DUMMY))
    case(entry, "C_tag without R_tag", BADARG, put("t.C_tag", DUMMY))
    case(entry, "R_tag beside R_ver", BADARG, *TAGS, TWIN)
    case(entry, "tags, doubled table of 2^32 bytes", BADARG, *TAGS, BIG_TWIN)
    case(entry, "d_model -1", BADARG, put("t.d_model", -1))
    case(entry, "d_model d + 1", BADARG, put("t.d_model", D + 1))
    case(entry, "head 2", BADARG, put("h.head", 2))
    case(entry, "workspace one byte short", WORKSPACE, put("ws_bytes", lambda c: c.ws_bytes - 1))
    # a twinned table and a fault behind it: nothing brings the table home before the call is refused
    case(entry, "twinned, null ws", BADARG, TWIN, put("ws", None))
    case(entry, "twinned, workspace one byte short", WORKSPACE, TWIN, put("ws_bytes", lambda c: c.ws_bytes - 1))


def optimizer(entry, sides, opts, also=()):
    """Every clause of check_optimizer on `sides` (1: the row side's slots alone) for each optimizer it tells apart."""
    rows, cols = ("R", "br"), (("C", "bc") if sides & 2 else ())
    for opt, name in opts:
        on = (put("h.optimizer", opt),) + tuple(also)
        betas = opt in (ADAMAX, NADAM, ADAM, LAZYADAM)
        for s in rows + cols:
            case(entry, "%s, null s1_%s" % (name, s), BADARG, *on, put("t.s1_" + s, None))
            if betas or opt in (ADADELTA, FTRL):
                case(entry, "%s, null s2_%s" % (name, s), BADARG, *on, put("t.s2_" + s, None))
        if betas:
            for f in ("beta1", "beta2"):
                for v in (0.0, 1.0):
                    case(entry, "%s, %s %g" % (name, f, v), BADARG, *on, put("h." + f, v))
        if opt in (ADADELTA, RMSPROP):
            for v in (0.0, 1.0):
                case(entry, "%s, rho %g" % (name, v), BADARG, *on, put("h.rho", v))
        if opt == FTRL:
            case(entry, "Ftrl, learning_rate 0", BADARG, *on, put("h.learning_rate", 0.0))
        if opt == SGD:
            for v in (-0.5, 1.0):
                case(entry, "SGD, momentum %g" % v, BADARG, *on, put("h.momentum", v))


ALL_OPTS = ((ADAGRAD, "Adagrad"), (SGD, "SGD"), (RMSPROP, "RMSprop"), (ADAMAX, "Adamax"), (ADAM, "Adam"), (ADADELTA, "Adadelta"),
            (FTRL, "Ftrl"), (NADAM, "Nadam"), (LAZYADAM, "LazyAdam"), (ROWWISE, "RowWiseAdagrad"))
SLOTS1 = ("s1_R", "s1_C", "s1_br", "s1_bc")

for e in ("glove_passes_f32", "glove_rowpass_f32", "glove_colpass_f32", "glove_apply_adagrad_f32", "glove_dense_grad_f32",
          "glove_pack_grad_f32", "glove_passes_packing_f32", "glove_pack_rest_f32", "glove_step_adagrad_f32",
          "glove_rowside_step_adagrad_f32", "glove_steps_adagrad_f32", "glove_step_adam_f32", "glove_step_sparse_f32",
          "glove_rowside_step_f32", "glove_steps_adam_f32"):
    common(e)

for s in SLOTS1:
    case("glove_apply_adagrad_f32", "null " + s, BADARG, put("t." + s, None))
case("glove_dense_grad_f32", "null G_flat", BADARG, put("G_flat", None))

for e in ("glove_pack_grad_f32", "glove_passes_packing_f32", "glove_pack_rest_f32"):
    for plan in ("rec", "pairs"):
        if e == "glove_passes_packing_f32" and plan == "pairs":
            continue                # (without records it is the plain passes: nothing is packed)
        case(e, "null packed", BADARG, put("packed", None), plan=plan)
        case(e, "capacity one entry short", WORKSPACE, put("capacity", lambda c: c.capacity - 1), plan=plan)
        case(e, "row side alone, capacity one entry short", WORKSPACE, put("h.sides", 1),
             put("capacity", lambda c: c.entries_needed() - 1), plan=plan)

e = "glove_loss_partials_f32"
for name in ("p", "t", "ws", "out4"):
    case(e, "null " + name, BADARG, put(name, None))
case(e, "d 0", BADARG, put("t.d", 0))
case(e, "d 6", BADARG, put("t.d", 6))
case(e, "d 1028", WORKSPACE, put("t.d", 1028))          # (the workspace of d = 8 is judged first)
case(e, "d 1028, its workspace", BADARG, put("t.d", 1028), put("ws_bytes", 1 << 40))
case(e, "workspace one byte short", WORKSPACE, put("ws_bytes", lambda c: c.ws_bytes - 1))


def packed_common(entry):
    for name in ("t", "G_flat", "mark"):
        case(entry, "null " + name, BADARG, put(name, None))
    for name, edit in (("V 0", put("t.V", 0)), ("d 0", put("t.d", 0)), ("d 6", put("t.d", 6)), ("d 1028", put("t.d", 1028)),
                       ("capacity -1", put("capacity", -1)), ("null lists", put("lists_null", True))):
        case(entry, name, BADARG, edit)
    for name, edit in (("null entries", bad_list(0, "entries", None)), ("neither header nor n", bad_list(0, "header", None)),
                       ("side -2", bad_list(0, "side", -2)), ("side 2", bad_list(0, "side", 2))):
        case(entry, "list 0: " + name, BADARG, edit)


packed_common("glove_combine_packed_f32")
case("glove_combine_packed_f32", "tag -1", BADARG, put("tag", -1))
for e in ("glove_count_packed_f32", "glove_apply_packed_adagrad_f32"):
    packed_common(e)
    case(e, "n_lists 0", BADARG, put("n_lists", 0))
    case(e, "list 1: null entries", BADARG, bad_list(1, "entries", None))
    case(e, "nine lists, list 8: null entries", BADARG, put("n_lists", 9), bad_list(8, "entries", None))
case("glove_count_packed_f32", "n_lists 256", BADARG, put("n_lists", MARK_COUNT_MASK + 1))
e = "glove_apply_packed_adagrad_f32"
case(e, "null h", BADARG, put("h", None))
for f in ("R", "C", "br", "bc", "scalars"):
    case(e, "null t." + f, BADARG, put("t." + f, None))
case(e, "optimizer -1", BADARG, put("h.optimizer", -1))
case(e, "optimizer 10", BADARG, put("h.optimizer", 10))
optimizer(e, 3, ALL_OPTS)
case(e, "sweep_sides -1", BADARG, put("h.sweep_sides", -1))
case(e, "sweep_sides 4", BADARG, put("h.sweep_sides", 4))
case(e, "Adam, list 1: null entries", BADARG, put("h.optimizer", ADAM), bad_list(1, "entries", None))
case(e, "twinned, sweep_sides 4", BADARG, TWIN, put("h.sweep_sides", 4))

e = "glove_gather_rows_f32"
case(e, "n -1", BADARG, put("n_rows", -1))
for d in (0, 6, 1028):
    case(e, "d %d" % d, BADARG, put("t.d", d))
for f in ("t.R", "t.br", "ids", "rows", "biases"):
    case(e, "null " + f.rpartition(".")[2], BADARG, put(f, None))

e = "glove_canonicalize_f32"
case(e, "null t", BADARG, put("t", None))
for f in ("R", "br"):
    case(e, "null " + f, BADARG, put("t." + f, None))
case(e, "V 0", BADARG, put("t.V", 0))
for d in (0, 6, 1028):
    case(e, "d %d" % d, BADARG, put("t.d", d))
case(e, "R_tag without C_tag", BADARG, put("t.R_ver", None), put("t.R_tag", DUMMY))
case(e, "R_tag beside R_ver", BADARG, *TAGS)
for f in ("C", "bc"):
    case(e, "tags, null " + f, BADARG, put("t.R_ver", None), *TAGS, put("t." + f, None))

for e, adam in (("glove_dense_adagrad_f32", False), ("glove_dense_adam_f32", True)):
    for name in ("t", "h", "G_flat"):
        case(e, "null " + name, BADARG, put(name, None))
    for name, edit in (("V 0", put("t.V", 0)), ("d 0", put("t.d", 0)), ("d 6", put("t.d", 6)), ("d_model -1", put("t.d_model", -1)),
                       ("d_model d + 1", put("t.d_model", D + 1))):
        case(e, name, BADARG, edit)
    for f in ("R", "C", "br", "bc", "scalars", "step") + SLOTS1 + (("s2_R", "s2_C", "s2_br", "s2_bc") if adam else ()):
        case(e, "null " + f, BADARG, put("t." + f, None))
    case(e, "RowWiseAdagrad", BADARG, put("h.optimizer", ROWWISE))
    case(e, "twinned, null G_flat", BADARG, TWIN, put("G_flat", None))
e = "glove_dense_adam_f32"
case(e, "LazyAdam", BADARG, put("h.optimizer", LAZYADAM))
for f in ("beta1", "beta2"):
    for v in (0.0, 1.0):
        case(e, "%s %g" % (f, v), BADARG, put("h." + f, v))
for v in (0.0, 1.0):
    case(e, "RMSprop, rho %g" % v, BADARG, put("h.optimizer", RMSPROP), put("h.rho", v))
case(e, "RMSprop, null s1_R", BADARG, put("h.optimizer", RMSPROP), put("t.s1_R", None))

# ---- the steps
for e in ("glove_step_adagrad_f32", "glove_steps_adagrad_f32"):
    for form in (-1, 6):
        case(e, "step_form %d" % form, BADARG, put("h.step_form", form))
    case(e, "twin form without R_ver", BADARG, put("h.step_form", FUSED_TWIN))
    case(e, "tagged form without tags", BADARG, put("h.step_form", TAGGED))
    for s in SLOTS1:
        for form, name in ((0, "auto"), (TWO_LAUNCH, "two-launch"), (ONE_PASS, "one-pass"), (THREE_LAUNCH, "three-launch")):
            case(e, "%s form, null %s" % (name, s), BADARG, put("h.step_form", form), put("t." + s, None))
        case(e, "twin form, null " + s, BADARG, TWIN, put("h.step_form", FUSED_TWIN), put("t." + s, None))
        case(e, "tagged form, null " + s, BADARG, *TAGS, put("h.step_form", TAGGED), put("t." + s, None))
        case(e, "two-launch form on pair arrays, null " + s, BADARG, put("t." + s, None), plan="pairs")
    case(e, "twin form, workspace one byte short", WORKSPACE, TWIN, put("h.step_form", FUSED_TWIN), put("ws_bytes", lambda c: c.ws_bytes - 1))
    case(e, "tagged form, no room for a chain record", WORKSPACE, *TAGS, put("h.step_form", TAGGED), put("ws_bytes", 16))
    case(e, "tagged form, null ws", BADARG, *TAGS, put("h.step_form", TAGGED), put("ws", None))
    case(e, "tagged form, head 2", BADARG, *TAGS, put("h.step_form", TAGGED), put("h.head", 2))

e = "glove_rowside_step_adagrad_f32"
for sides in (0, 2, 3):
    case(e, "sides %d" % sides, BADARG, put("h.sides", sides))
for s in SLOTS1:
    case(e, "null " + s, BADARG, put("t." + s, None))
    case(e, "null " + s, BADARG, put("t." + s, None), plan="pairs")

for e in ("glove_step_adam_f32", "glove_steps_adam_f32"):
    case(e, "null G_flat", BADARG, put("G_flat", None))
    optimizer(e, 3, ((ADAM, "Adam"),))
    # (one side alone takes the dense form: passes, dense gradient, dense sweep)
    case(e, "dense form, null G_flat", BADARG, put("h.sides", 1), put("G_flat", None))
    case(e, "dense form, null s2_R", BADARG, put("h.sides", 1), put("t.s2_R", None))
    case(e, "dense form, beta1 0", BADARG, put("h.sides", 1), put("h.beta1", 0.0))
    case(e, "dense form, LazyAdam", BADARG, put("h.sides", 1), put("h.optimizer", LAZYADAM))
    # (tags, records and id bitmaps: the one-launch form)
    case(e, "one-launch form, null s2_C", BADARG, *TAGS, put("t.s2_C", None))
    case(e, "one-launch form, beta2 1", BADARG, *TAGS, put("h.beta2", 1.0))
    case(e, "one-launch form, no room for a chain record", WORKSPACE, *TAGS, put("ws_bytes", 16))
    case(e, "one-launch form, null ws", BADARG, *TAGS, put("ws", None))

for e in ("glove_steps_adagrad_f32", "glove_steps_adam_f32"):
    case(e, "null plans", BADARG, put("plans_null", True))
    case(e, "n -1", BADARG, put("n_plans", -1))
    case(e, "null first plan", BADARG, put("plan0_null", True))
    case(e, "two plans, null first plan", BADARG, put("n_plans", 2), put("plan0_null", True))

e = "glove_step_sparse_f32"
case(e, "optimizer -1", BADARG, put("h.optimizer", -1))
case(e, "optimizer 10", BADARG, put("h.optimizer", 10))
for sides in (1, 2):
    case(e, "sides %d" % sides, BADARG, put("h.sides", sides))
optimizer(e, 3, ALL_OPTS)
for opt, name in ((RMSPROP, "RMSprop"), (NADAM, "Nadam"), (ADAM, "Adam")):
    case(e, name + ", null G_flat", BADARG, put("h.optimizer", opt), put("G_flat", None))
case(e, "Adagrad, step_form 6", BADARG, put("h.optimizer", ADAGRAD), put("h.step_form", 6))

e = "glove_rowside_step_f32"
for sides in (0, 2, 3):
    case(e, "sides %d" % sides, BADARG, put("h.sides", sides))
case(e, "optimizer -1", BADARG, put("h.optimizer", -1))
case(e, "optimizer 10", BADARG, put("h.optimizer", 10))
optimizer(e, 1, ALL_OPTS)
for opt, name in ((ADAM, "Adam"), (NADAM, "Nadam")):       # (their fused kernel asks for both sides' slots)
    for s in ("s1_C", "s1_bc", "s2_C", "s2_bc"):
        case(e, "%s, null %s" % (name, s), BADARG, put("h.optimizer", opt), put("t." + s, None))
for opt, name in ((RMSPROP, "RMSprop"), (NADAM, "Nadam"), (ADAM, "Adam")):
    case(e, name + ", null G_flat", BADARG, put("h.optimizer", opt), put("G_flat", None))
for s in ("s1_C", "s1_bc"):                                 # (its dense sweep's segments cover all four tables)
    case(e, "RMSprop, null " + s, BADARG, put("h.optimizer", RMSPROP), put("t." + s, None))
for opt, name in ((RMSPROP, "RMSprop"), (LAZYADAM, "LazyAdam"), (ADAM, "Adam")):
    case(e, name + ", workspace one byte short", WORKSPACE, put("h.optimizer", opt), put("ws_bytes", lambda c: c.ws_bytes - 1))

assert len({case_id(c) for c in CASES}) == len(CASES), "case ids are unique"

# (see the module's docstring) variant -> the entry points, without glove_ and _f32, whose refusal of it came behind a launch.
# Recorded from the CPU run against the library as it was, but for the three bad lists of the packed entry points: a failed
# launch there went unnoticed in front of the refusal, read off the source.
_ALL = ("passes", "rowpass", "colpass", "apply_adagrad", "dense_grad", "passes_packing", "rowside_step_adagrad", "step_sparse",
        "rowside_step")
_STEPS = ("step_adagrad", "steps_adagrad", "step_adam", "steps_adam")
_ADAGRAD, _ADAM = _STEPS[:2], _STEPS[2:]
_SLOTS = ["%s, null %s" % (form, s) for s in SLOTS1 for form in ("auto form", "two-launch form")]
PARENT_LAUNCHED = frozenset("glove_%s_f32:%s" % (e, name) for name, entries in {
    "R_ver, doubled table of 2^32 bytes": _ALL + _STEPS,
    "tags, doubled table of 2^32 bytes": _ALL,
    "twinned, null ws": _ALL + _STEPS,
    "twinned, workspace one byte short": _ALL + _STEPS + ("pack_grad", "pack_rest"),
    "twinned, null G_flat": ("dense_adagrad", "dense_adam"),
    **{name: _ADAGRAD for name in _SLOTS},
    **{"two-launch form on pair arrays, null %s@pairs" % s: _ADAGRAD for s in SLOTS1},
    **{"null %s@pairs" % s: ("rowside_step_adagrad",) for s in SLOTS1},
    **{"Adagrad, null " + s: ("step_sparse",) for s in SLOTS1},
    "RMSprop, null s1_C": ("rowside_step",), "RMSprop, null s1_bc": ("rowside_step",),
    **{"dense form, " + what: _ADAM for what in ("null G_flat", "null s2_R", "beta1 0", "LazyAdam")},
    "Adam, list 1: null entries": ("apply_packed_adagrad",),
    "nine lists, list 8: null entries": ("apply_packed_adagrad", "count_packed"),
}.items() for e in entries)


def base_calls():
    """(entry, plan kind, edits) of the valid call every variant of an entry point starts from."""
    return [(e, plan, BASE.get(e, ())) for e in ENTRIES for plan in ("rec", "pairs")]


def run(lib, entry, env, edits, plan="rec"):
    """The code `entry` answers the base call with `edits` applied."""
    c = Call(env, plan)
    for edit in edits:
        edit(c)
    return getattr(lib, entry)(*ENTRIES[entry](c))


def fake_plan(ptr, records, counts=(B, B, B, B, 0, 0, 0, 0)):
    """A GlovePlan sized like trainer.hip_api.Plan(B, V, CHUNK_CAP) with every array at `ptr` (the CPU test; the GPU test
    takes a real plan's struct)."""
    p = GlovePlan()
    p.B, p.chunk_cap, p.cap_chunks, p.cap_uniq, p.heavy_chunks = B, CHUNK_CAP, B, min(B, V), 8
    p.cap_heavy = 2 * B // (8 * CHUNK_CAP) + 2
    for i, n in enumerate(counts):
        p.host_counts[i] = n
    for f in ("counts", "r_partner", "r_w", "r_y", "r_to_c", "r_chunk_id", "r_chunk_start", "r_uniq_slot", "r_uniq_rec", "c_partner",
              "c_perm", "c_w", "c_y", "c_chunk_id", "c_chunk_start", "c_uniq_slot", "c_uniq_rec", "heavy", "r_mark", "c_mark"):
        setattr(p, f, ptr)
    if records:
        p.r_crec = p.c_crec = ptr
    return p
