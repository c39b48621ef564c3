import os
import sys

import pytest
# torch first, before any test loads peps_amd/lib/libpepsgpu.so: torch's libamdhip64.so carries the soname libamdhip64.so.7,
# so loaded first it is the one HIP runtime of the session; loaded after the library it comes in as a second runtime, and
# the two do not share the device (the runtime that came second finds no GPU): the suite's outcome would hang on test order
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = os.path.join(GOLDEN, "ref_fixtures")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def fixtures_dir():
    return FIXTURES
