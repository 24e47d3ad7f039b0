"""The step library's refusals on the GPU (tests/step_refusal_cases.py): every variant over the device buffers of a real plan
and real tables answers its code and leaves every buffer as it was, bit for bit.  Only refused calls run here — that each
of them is refused before anything is launched is what tests/test_step_refusals.py shows on a machine without a GPU, where
the base calls are shown to be accepted as well."""
import numpy as np
import pytest
import torch

import step_refusal_cases as cases

pytestmark = pytest.mark.gpu


class Buffers:
    def __init__(self, hip):
        from trainer.hip_api import DeviceTables, _ptr
        rng = np.random.default_rng(5)
        dev = lambda a: torch.from_numpy(a).cuda()
        row, col = (dev(rng.integers(0, cases.V, cases.B).astype(np.int32)) for _ in range(2))
        w, y = (dev(rng.random(cases.B, dtype=np.float32)) for _ in range(2))
        self.plans, structs = {}, {}
        for kind, records in (("rec", True), ("pairs", False)):
            plan = hip.build_plan(row, col, w, y, cases.V, chunk_cap=cases.CHUNK_CAP, records=records)
            plan.host_counts = [int(x) for x in plan.counts.tolist()]
            plan._struct = None
            self.plans[kind], structs[kind] = plan, plan.struct()
        assert structs["rec"].r_crec and structs["rec"].r_partner and not structs["pairs"].r_crec
        self.tables = DeviceTables(cases.V, cases.D, "Adam", seed=3)        # both slots
        assert self.tables.d == cases.D
        ws_bytes = hip.lib.glove_step_workspace_bytes(cases.B, self.plans["rec"].cap_chunks, cases.D)
        noise = lambda n: torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(n))
        sizes = {"ws": ws_bytes, "G_flat": 4 * hip.lib.glove_dense_grad_layout(0, cases.V, cases.D, None), "loss_out": 16,
                 "packed": 4 * (1 + 2 * cases.B) * (cases.D + 4), "mark": 4 * 2 * cases.V, "out4": 16, "ids": 16,
                 "rows": 4 * 3 * cases.D, "biases": 16, "dummy": 256}
        self.raw = {k: noise(n) for k, n in sizes.items()}
        self.env = cases.Env(structs, self.tables.struct(), {k: _ptr(v) for k, v in self.raw.items()}, ws_bytes,
                             torch.cuda.current_stream().cuda_stream)

    def state(self):
        t = self.tables
        held = [t._R, t._C, t._br, t._bc, t.scalars, t.step] + [s[n] for s in (t.s1, t.s2) for n in t.NAMES] + list(self.raw.values())
        for p in self.plans.values():
            held += [p.counts, p.r_chunk_start, p.c_chunk_start]
        return torch.cat([x.contiguous().view(torch.uint8).flatten() for x in held])


@pytest.fixture(scope="module")
def bufs(hip):
    return Buffers(hip)


@pytest.mark.parametrize("entry", list(cases.ENTRIES))
def test_refused_calls_touch_nothing(hip, bufs, entry):
    mine = [c for c in cases.CASES if c.entry == entry]
    assert mine
    before = bufs.state().clone()
    for c in mine:
        # (one at a time: a call that is not refused has been handed a null or short buffer)
        assert cases.run(hip.lib, c.entry, bufs.env, c.edits, c.plan) == c.code, cases.case_id(c)
        assert torch.equal(bufs.state(), before), cases.case_id(c)
