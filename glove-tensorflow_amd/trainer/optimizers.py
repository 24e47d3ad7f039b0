"""The optimizer names the trainer knows and what each one needs on the host: ONE record per name.  Everything in trainer/
that depends on the name — the GLOVE_OPT_* code, the slot layout of DeviceTables, the exchange a multi-rank step may take,
the entry point of the single-GPU step, the scratch of the row-side step — reads it here; a new name is one new record.
What the names compute is the library's business (include/glove_hip.h glove_hyper.optimizer).  No torch here."""
from __future__ import annotations

from dataclasses import dataclass
from types import MappingProxyType as _frozen


@dataclass(frozen=True)
class Optimizer:
    name: str
    code: int                       # glove_hyper.optimizer (GLOVE_OPT_*)
    defaults: _frozen               # the Keras-legacy default config: what train_utils.get_optimizer returns
    keras: bool = True              # `tf.keras.optimizers.get` resolves the name (reference train_utils.py:13-16); False: this build's addition
    about: str = ""                 # ... and then what it is, for the --optimizer help
    # ---- DeviceTables: slots and scalars at step 0
    slot1_init: float = 0.0         # 0.1: initial_accumulator_value (Keras default); zeros: m, momentum accumulator, rms, accum_grad
    slot2: bool = False             # v (Adam, Adamax, Nadam, LazyAdam), accum_var (Adadelta), linear (Ftrl)
    row_wise: bool = False          # slot 1 of R and C is ONE float per row (float[rows]), not shaped like the table
    scalars: tuple = (0.0,) * 8     # glove_tables.scalars: [1] the global bias's accumulator, [4], [5] Nadam's momentum cache
    # ---- several ranks
    exchange: str = "rows"          # "rows": only touched rows move, the lists carry the union of the ranks' ids; "dense": every row's slots move every step, dense all-reduce; "either"
    dense_apply: str | None = None  # the GloveHip wrapper that applies a dense gradient buffer (None: there is no dense apply)
    own_rowside: bool = False       # the row side of a sharded step has an entry point of its own (glove_rowside_step_adagrad_f32), not glove_rowside_step_f32
    row_scratch: str | None = None  # glove_rowside_step_f32's scratch: "marks" (V_row floats, the row ids are marked there), "row_half" (of the dense layout: the row gradients are summed there)
    # ---- one GPU
    entry: str = "sparse"           # the whole step is glove_step_<entry>_f32; "adagrad" and "adam" also have the chained glove_steps_<entry>_f32
    step_buffer: bool = False       # the step needs the dense gradient buffer (all zero between steps)
    dense_step: bool = False        # Stepper.step on one rank runs passes + dense_grad + dense_apply instead of `entry`
    tagged: bool = False            # the step has a one-launch form on step-tagged tables (DeviceTables.enable_tags) ...
    tagged_sweeps: bool = False     # ... which sweeps every row of both tables: set up only while 2 B <= V_row + V
    twinned: bool = False           # the fused step has a form on a twinned row table (DeviceTables.enable_twin)
    rho: float = 0.9                # glove_hyper.rho when the caller names none (the name's own Keras default)

    @property
    def chained(self) -> bool:
        return self.entry != "sparse"


_ADAM = _frozen({"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7})
_ADAGRAD = _frozen({"initial_accumulator_value": 0.1, "epsilon": 1e-7})
_ACC = (0.0, 0.1) + (0.0,) * 6     # the global bias's accumulator starts where the slots do

OPTIMIZERS = _frozen({o.name: o for o in (
    Optimizer("Adagrad", 0, _ADAGRAD, slot1_init=0.1, scalars=_ACC, exchange="either", dense_apply="dense_adagrad", own_rowside=True, entry="adagrad", tagged=True, twinned=True),
    Optimizer("SGD", 1, _frozen({"momentum": 0.0, "nesterov": False})),
    Optimizer("RMSprop", 2, _frozen({"rho": 0.9, "momentum": 0.0, "epsilon": 1e-7, "centered": False}), exchange="dense", dense_apply="dense_adam", row_scratch="row_half", step_buffer=True),
    Optimizer("Adamax", 3, _ADAM, slot2=True),
    Optimizer("Adam", 4, _ADAM, slot2=True, exchange="dense", dense_apply="dense_adam", row_scratch="marks", entry="adam", step_buffer=True, dense_step=True, tagged=True, tagged_sweeps=True),
    Optimizer("Adadelta", 5, _frozen({"rho": 0.95, "epsilon": 1e-7}), slot2=True, rho=0.95),
    Optimizer("Ftrl", 6, _frozen({"learning_rate_power": -0.5, "initial_accumulator_value": 0.1, "l1_regularization_strength": 0.0,
                                  "l2_regularization_strength": 0.0, "l2_shrinkage_regularization_strength": 0.0, "beta": 0.0}),
              slot1_init=0.1, slot2=True, scalars=_ACC),
    # (m, v decay everywhere, touched rows move: the lists ARE the union of the ranks' ids — the rows no list names decay in a sweep in front of the apply; scalars: the momentum cache, a Keras optimizer weight initialised to ones)
    Optimizer("Nadam", 7, _frozen(dict(_ADAM, schedule_decay=0.004)), slot2=True, scalars=(0.0,) * 4 + (1.0, 1.0, 0.0, 0.0), row_scratch="marks", step_buffer=True),
    Optimizer("LazyAdam", 8, _ADAM, keras=False, about="Adam on the rows a batch touches only", slot2=True),
    Optimizer("RowWiseAdagrad", 9, _ADAGRAD, keras=False, about="Adagrad with one accumulator per embedding row", slot1_init=0.1, row_wise=True, scalars=_ACC),
)})
BY_CODE = _frozen({o.code: o for o in OPTIMIZERS.values()})


def names(keep=lambda o: True) -> tuple:
    """The names whose record `keep` accepts, in the order of their codes."""
    return tuple(o.name for o in OPTIMIZERS.values() if keep(o))
