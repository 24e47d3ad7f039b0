"""The step library's refusals on a machine without a GPU (tests/step_refusal_cases.py): there a launch fails with a HIP error
code > 0 and touches nothing, so the structs can stand over host dummies.  Every base call must come back > 0 (accepted, up
to its first launch), every variant with its GLOVE_E_* code — and so, refused before anything was launched.  With a GPU this
file has nothing to say: tests/test_gpu_step_refusals.py runs the same table over device buffers."""
import ctypes as C

import pytest

import step_refusal_cases as cases


@pytest.fixture(scope="module")
def lib():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU would run the accepted calls: tests/test_gpu_step_refusals.py")
    from trainer import hip_api
    if not hip_api.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_library()


@pytest.fixture(scope="module")
def env(lib):
    from trainer.hip_api import GloveTables
    host = C.create_string_buffer(1 << 20)      # zeros; nothing reads them: every launch fails
    ptr = C.addressof(host)
    t = GloveTables()
    t.V, t.d = cases.V, cases.D
    for f, _ in GloveTables._fields_[4:18]:     # R .. step
        setattr(t, f, ptr)
    names = ("ws", "G_flat", "loss_out", "packed", "mark", "out4", "ids", "rows", "biases", "dummy")
    e = cases.Env({"rec": cases.fake_plan(ptr, True), "pairs": cases.fake_plan(ptr, False)}, t, dict.fromkeys(names, ptr),
                  lib.glove_step_workspace_bytes(cases.B, cases.B, cases.D))
    e.keep = host
    assert 0 < e.ws_bytes <= len(host)
    return e


@pytest.mark.parametrize("entry,plan,edits", cases.base_calls(), ids=lambda v: v if isinstance(v, str) else "")
def test_base_call_is_accepted(lib, env, entry, plan, edits):
    assert cases.run(lib, entry, env, edits, plan) > 0


@pytest.mark.parametrize("entry", list(cases.ENTRIES))
def test_variants_are_refused_before_any_launch(lib, env, entry):
    mine = [c for c in cases.CASES if c.entry == entry]
    assert mine
    got = {cases.case_id(c): cases.run(lib, c.entry, env, c.edits, c.plan) for c in mine}
    assert got == {cases.case_id(c): c.code for c in mine}


def test_parent_launched_names_cases():
    assert cases.PARENT_LAUNCHED <= {cases.case_id(c) for c in cases.CASES}
