"""Randomised differential test: HIP engine vs CPU oracle on small synthetic worlds with parameter sets drawn at
random (light algorithms, speed ranges with power-of-two and non-power-of-two spans, awareness range, replanning
thresholds, contraflow switches, stranding chances, penalties, rain with a manager, transition timers, stuck despawn,
field-of-view masking, fractional road-type penalties, the non-batched step path).  Every
tick is compared state for state; the draws are seeded, so a failure names its case."""
import os

import pytest

from tests.random_cases import run_case

pytestmark = pytest.mark.gpu


N_CASES = int(os.environ.get("TS_RANDOM_CASES", "20"))   # more for a bug hunt: TS_RANDOM_CASES=200 TS_RANDOM_TICKS=80
FIRST = int(os.environ.get("TS_RANDOM_FIRST", "0"))
N_TICKS = int(os.environ.get("TS_RANDOM_TICKS", "45"))


@pytest.mark.parametrize("case", range(FIRST, FIRST + N_CASES))
def test_hip_vs_oracle_random_config(case):
    from oracle import pyoracle
    from trafficsimulation_amd._lib import new_engine
    run_case(case, lambda: (new_engine(), pyoracle.load()), ticks=N_TICKS)
