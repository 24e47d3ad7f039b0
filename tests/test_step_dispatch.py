"""The optimizer table (trainer/optimizers.py) against independent statements of what it must say, and the entry points a
step of every name reaches against the committed call traces (tests/golden/step_call_traces.json, written by
tests/golden/make_step_traces.py before the table existed).  All on the CPU: the traces are pure host logic."""
import importlib.util
import json
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden"

NAMES = ("Adagrad", "SGD", "RMSprop", "Adamax", "Adam", "Adadelta", "Ftrl", "Nadam", "LazyAdam", "RowWiseAdagrad")
HEADER_NAMES = {"ADAGRAD": "Adagrad", "SGD": "SGD", "RMSPROP": "RMSprop", "ADAMAX": "Adamax", "ADAM": "Adam", "ADADELTA": "Adadelta",
                "FTRL": "Ftrl", "NADAM": "Nadam", "LAZYADAM": "LazyAdam", "ROWWISE_ADAGRAD": "RowWiseAdagrad"}

# what DeviceTables(12, 8, name, device="cpu", seed=0) holds at step 0, written out: (slot-1 value, slot 2 exists,
# the table slots are one float per row, scalars)
ZEROS = [0.0] * 8
ACC = [0.0, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
TABLES_AT_STEP_0 = {
    "Adagrad": (0.1, False, False, ACC),
    "SGD": (0.0, False, False, ZEROS),
    "RMSprop": (0.0, False, False, ZEROS),
    "Adamax": (0.0, True, False, ZEROS),
    "Adam": (0.0, True, False, ZEROS),
    "Adadelta": (0.0, True, False, ZEROS),
    "Ftrl": (0.1, True, False, ACC),
    "Nadam": (0.0, True, False, [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]),
    "LazyAdam": (0.0, True, False, ZEROS),
    "RowWiseAdagrad": (0.1, False, True, ACC),
}


def test_codes_are_the_headers():
    from trainer.hip_api import OPTIMIZER_CODES
    from trainer.optimizers import OPTIMIZERS
    text = (REPO / "include" / "glove_hip.h").read_text()
    header = {HEADER_NAMES[m.group(1)]: int(m.group(2)) for m in re.finditer(r"^#define GLOVE_OPT_(\w+) (\d+)\s*$", text, re.M)}
    assert len(header) == 10 and set(header) == set(NAMES)
    assert dict(OPTIMIZER_CODES) == header
    assert tuple(OPTIMIZERS) == NAMES and {n: o.code for n, o in OPTIMIZERS.items()} == header
    assert all(o.name == n for n, o in OPTIMIZERS.items())


@pytest.mark.parametrize("name", NAMES)
def test_tables_at_step_0(name):
    import torch
    from trainer.hip_api import DeviceTables
    s1, has_s2, row_wise, scalars = TABLES_AT_STEP_0[name]
    dt = DeviceTables(12, 8, name, device="cpu", seed=0)
    shapes = {"R": (12, 8), "C": (12, 8), "br": (12,), "bc": (12,)}
    slot1_shapes = dict(shapes, R=(12,), C=(12,)) if row_wise else shapes
    assert set(dt.s1) == set(shapes) and set(dt.s2) == (set(shapes) if has_s2 else set())
    for n, shape in shapes.items():
        assert tuple(getattr(dt, n).shape) == shape
        assert tuple(dt.s1[n].shape) == slot1_shapes[n] and dt.s1[n].dtype == torch.float32
        assert torch.equal(dt.s1[n], torch.full(slot1_shapes[n], s1, dtype=torch.float32)), n
        if has_s2:
            assert tuple(dt.s2[n].shape) == shape and dt.s2[n].dtype == torch.float32
            assert int(torch.count_nonzero(dt.s2[n])) == 0, n
    assert dt.scalars.dtype == torch.float32 and tuple(dt.scalars.shape) == (8,)
    np.testing.assert_array_equal(dt.scalars.numpy(), np.asarray(scalars, dtype=np.float32))
    assert dt.global_step == 0 and dt.R_tag is None and dt.R_ver is None


def test_derived_tuples():
    from trainer import hip_api, stepper, train_utils
    assert stepper.Stepper.ROWS_ONLY == ("SGD", "Adamax", "Adadelta", "Ftrl", "Nadam", "LazyAdam", "RowWiseAdagrad")
    assert stepper.Stepper.DENSE_ONLY == ("RMSprop", "Adam")             # (in the order of the codes, like every derived tuple)
    assert stepper.KERAS_OPTIMIZERS == ("Adagrad", "SGD", "RMSprop", "Adamax", "Adam", "Adadelta", "Ftrl", "Nadam")
    assert stepper.SHARDED_OPTIMIZERS == stepper.KERAS_OPTIMIZERS + ("LazyAdam", "RowWiseAdagrad")
    assert hip_api.ROW_WISE_OPTIMIZERS == ("RowWiseAdagrad",)
    assert train_utils.OPTIMIZERS == {          # the Keras-legacy defaults, written out
        "Adagrad": {"initial_accumulator_value": 0.1, "epsilon": 1e-7},
        "Adam": {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7},
        "LazyAdam": {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7},
        "RowWiseAdagrad": {"initial_accumulator_value": 0.1, "epsilon": 1e-7},
        "SGD": {"momentum": 0.0, "nesterov": False},
        "RMSprop": {"rho": 0.9, "momentum": 0.0, "epsilon": 1e-7, "centered": False},
        "Adamax": {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7},
        "Nadam": {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "schedule_decay": 0.004},
        "Adadelta": {"rho": 0.95, "epsilon": 1e-7},
        "Ftrl": {"learning_rate_power": -0.5, "initial_accumulator_value": 0.1, "l1_regularization_strength": 0.0,
                 "l2_regularization_strength": 0.0, "l2_shrinkage_regularization_strength": 0.0, "beta": 0.0},
    }
    assert train_utils.get_optimizer("lazyadam", learning_rate=0.01) == {
        "class_name": "LazyAdam", "config": {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "learning_rate": 0.01}}


def test_the_table_imports_no_torch():
    text = (REPO / "glove-tensorflow_amd" / "trainer" / "optimizers.py").read_text()
    assert not re.search(r"^\s*(import|from)\s+torch\b", text, re.M)


def test_default_rho_is_the_names_own():
    from trainer.hip_api import make_hyper
    for name in NAMES:
        assert make_hyper(batch_size=4, optimizer=name).rho == np.float32(0.95 if name == "Adadelta" else 0.9)
    assert make_hyper(batch_size=4, optimizer=5).rho == np.float32(0.95)        # (a code instead of a name)
    assert make_hyper(batch_size=4, optimizer="Adadelta", rho=0.5).rho == 0.5


def test_step_call_traces_are_the_committed_ones():
    """Which C entry point a step of every name reaches — through Stepper and RowShardedStepper on one rank, through the
    row-sharded form's exchanges, HipBackend.rowside_step and HipBackend.apply_dense — and with which hyper.sides,
    hyper.optimizer, null / non-null G_flat and loss_out, plan count and tagged / twinned tables: equal to the file."""
    spec = importlib.util.spec_from_file_location("make_step_traces", GOLDEN / "make_step_traces.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    got = json.loads(json.dumps(gen.build_traces()))
    want = json.loads((GOLDEN / "step_call_traces.json").read_text())
    assert set(got["cases"]) == set(want["cases"])
    for key in sorted(want["cases"]):
        assert got["cases"][key] == want["cases"][key], key
    assert got == want
