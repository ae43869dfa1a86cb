#!/usr/bin/env python
"""Generate tests/golden/signatures.json: (class, method, str(inspect.signature)) of every public callable of every class in
models.py, as tests/test_signatures_cpu.py lists them.  Run at the commit whose API is the one to keep (it was written at the parent of
the change that put the serving front end behind one row source); needs no GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import poi_amd                                           # noqa: E402,F401  (the alias of the package directory)
from tests.test_signatures_cpu import GOLDEN, public_signatures      # noqa: E402

with open(GOLDEN, "w") as f:
    json.dump(public_signatures(), f, indent=0)
    f.write("\n")
print("wrote", GOLDEN)
