"""Row-isolation checks (tests/isolation.py, tests/isolation_cases.py) on the device: the full table, at the widths of the
decode step, where the last-arriver hand-over of K1d + K5, the persistent K1w head hand-over, ``o_exchange`` and the paired
block ids of the full-head K2 really run concurrently.  Run with ``pytest -m gpu``."""
import pytest

import isolation as I
import isolation_cases as IC


@pytest.mark.gpu
@pytest.mark.parametrize("op", IC.table(gpu=True))
def test_isolation(hip, op):
    I.check_all(op, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("B,d,dtype", IC.REARM)
def test_isolation_rows_rearm(hip, B, d, dtype):
    IC.check_rows_rearm("cuda", B, d, dtype)
