"""The Python binding of the tracking and landing section makes the C calls, and returns the structures, that it made at the
commit tests/golden/binding_calls.json was recorded at: every public method, both memory forms, a handle whose z_stride (96)
is above n_nlp (95), so that the host forms pad, and one whose z_stride is n_nlp, the argument combinations of
tests/binding_calls.py and the refusals of the Python side.  The golden holds no number a kernel computed: symbols, which
buffer went where, the constants the binding staged, shapes and messages.
The arguments of a call stand in the order of its prototype in include/qln_evaluator.h.

Record (on the GPU, at the commit whose behaviour is the yardstick):
    python tests/test_gpu_binding_calls.py --record COMMIT [PATH]"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import binding_calls as BC  # noqa: E402

pytestmark = pytest.mark.gpu
FORMS = ("device", "host")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(BC.GOLDEN))["trace"]


@pytest.fixture(scope="module")
def trace():
    return BC.record()


def test_the_golden_covers_both_handles_and_forms(golden):
    assert sorted(golden) == sorted(BC.HANDLES)
    # B = 3, n_nlp = 95: the padded handle's Z has z_stride = 96 a problem, so the host forms' padding of (B, n_nlp) rows runs
    z = {kind: golden[kind][form]["tracking_rollout" + sfx + " | all"].rsplit("-> ", 1)[1]
         for kind in golden for form, sfx in (("host", "_host"),)}
    assert z == {"padded": "n[288]", "unpadded": "n[285]"}
    for kind, least in (("padded", 100), ("unpadded", 25)):
        assert sorted(golden[kind]) == sorted(FORMS)
        for form in FORMS:
            made = [v for v in golden[kind][form].values() if v.startswith("qln_") and "(not made)" not in v]
            assert len(made) >= least
            assert all(v.split("(")[0].endswith("_host") == (form == "host") for v in made)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", list(BC.HANDLES))
def test_same_calls_and_returns(golden, trace, kind, form):
    want, got = golden[kind][form], trace[kind][form]
    assert list(got) == list(want)
    for key in want:
        symbol = want[key].split("(")[0]
        assert got[key] == want[key], (key, BC.PARAMS.get(symbol))


if __name__ == "__main__":
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--record", __doc__
    doc = {"recorded_at": sys.argv[2], "trace": BC.record()}
    path = sys.argv[3] if len(sys.argv) == 4 else BC.GOLDEN
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    entries = [v for k in doc["trace"].values() for t in k.values() for v in t.items()]
    print(len(entries), "entries,", sum(" !! " in v for _, v in entries), "refusals ->", path)
    for k, v in entries:
        if " !! " in v and "refuse:" not in k and "rule:" not in k:
            print("  raised outside the refusal cases:", k, v)
