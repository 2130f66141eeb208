"""The Python binding keeps its surface: every public name of api, every public method of Context, every dataclass field
with its default, and the private names that tests and tools use, against the recording tests/data/api_surface.json
(tests/tools/api_record.py made it from the api.py before the binding's helpers were shared).  No GPU, no library."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record():
    spec = importlib.util.spec_from_file_location("api_record", os.path.join(ROOT, "tests", "tools", "api_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


with open(os.path.join(ROOT, "tests", "data", "api_surface.json")) as f:
    WANT = json.load(f)


@pytest.fixture(scope="module")
def got():
    return json.loads(json.dumps(record().surface()))


@pytest.mark.parametrize("part", ["names", "context", "dataclasses", "private"])
def test_surface(got, part):
    assert sorted(got[part]) == sorted(WANT[part])
    for k in WANT[part]:
        assert got[part][k] == WANT[part][k], k
