"""Every malformed argument of tests/tools/api_record.py's cases is refused as tests/data/api_rejects.json recorded it: the
same exception type, a message that names the method (where the recorded one did) and the argument, and all of it before the
first call into the library -- the context has no handle, and every library function raises ReachedLibrary when called."""
import json
import os

import pytest

from test_api_surface_cpu import ROOT, record

with open(os.path.join(ROOT, "tests", "data", "api_rejects.json")) as f:
    WANT = {(r["method"], r["case"]): r for r in json.load(f)}


@pytest.fixture(scope="module")
def got():
    return {(r["method"], r["case"]): r for r in record().run_cases()}


def test_same_cases(got):
    assert sorted(got) == sorted(WANT)


@pytest.mark.parametrize("key", sorted(WANT), ids=lambda k: f"{k[0]}-{k[1]}".replace(" ", "_"))
def test_reject(got, key):
    want, r = WANT[key], got[key]
    assert r["type"] not in ("ReachedLibrary", "AttributeError"), r["message"]
    assert r["type"] == want["type"], r["message"]
    assert want["argument"] in r["message"]
    if want["names_method"]:
        assert want["method"] in r["message"]
