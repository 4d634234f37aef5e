"""The value domain of the pointwise, pooling, optimizer, reduction and RNG kernels on the device (tests/POINTWISE_DOMAIN.md): every
case of tests/pointwise_domain.py against its numpy restatement -- NaN, +-inf, +-0, subnormals, the largest floats and exact ties.
A failing check names the probe: the operands of the first element that differs."""
import pytest

import pointwise_domain as PD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    c = get_context(0)
    math, fusion = c.get_math(), c.get_fusion()
    yield c
    c.set_math(math); c.set_fusion(fusion)


@pytest.mark.parametrize("case", PD.CASES, ids=[c.name for c in PD.CASES])
def test_value_domain(ctx, case):
    checks = PD.run_case(ctx, case)
    assert checks, case.name
    failures = []
    for c in checks:
        try:
            PD.verify(c)
        except AssertionError as e:
            failures.append(str(e))
    print("%s: %d checks, %d failed" % (case.name, len(checks), len(failures)))
    assert not failures, "%d of %d checks failed:\n%s" % (len(failures), len(checks), "\n".join(failures[:12]))
