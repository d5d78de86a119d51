#!/usr/bin/env python3
"""Writes tests/golden/plan_digests.json: the digests tests/test_layer_ops.py::test_plans_equal_the_recorded_ones compares with.
Record from a build of the commit the plans have to stay equal to, never from the code under test:

    NESTI_LIB=<that commit's libnesti_hip.so> python scripts/record_plan_digests.py

No GPU involved: nesti_debug_tower_ops and the two size entries are host code."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import _lib  # noqa: E402
from test_layer_ops import PLAN_GOLDEN, plan_digests  # noqa: E402

if not os.environ.get("NESTI_LIB"):
    sys.exit("set NESTI_LIB to the library of the commit to record from")
digests = plan_digests(_lib.load())
with open(PLAN_GOLDEN, "w") as f:
    json.dump(digests, f, indent=0, sort_keys=True)
    f.write("\n")
print("recorded %d digests from %s" % (len(digests), _lib.LIB_PATH))
