"""The evaluation kernels' results, bit for bit: PREDICT top-k, 3CosAdd, 3CosMul, the pair cosine, k-means assign and
update on the seeded cases of tests/golden/make_eval_bits.py give the digests of tests/golden/eval_kernel_bits.json,
which were recorded on the MI355X from a build of the commit before the three similarity GEMMs were moved onto one
tile loop (csrc/glove_sim_gemm.h), twice, with identical results.

The parity tests of these kernels compare with float64 at rtol 1e-5: they would not see a changed summation order.
A mismatch here means the arithmetic order of a kernel has changed — restore it; regenerating the file from the changed
code is not a fix."""
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_eval_bits  # noqa: E402

WANT = json.loads((GOLDEN / "eval_kernel_bits.json").read_text())["cases"]


def test_fixture_lists_the_cases():
    assert sorted(WANT) == sorted(make_eval_bits.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(make_eval_bits.CASES))
def test_eval_kernel_bits(hip, name):
    got = make_eval_bits.run_case(hip, name)
    print(name, {out: (g["head"], WANT[name][out]["head"]) for out, g in got.items()})
    assert got == WANT[name]
