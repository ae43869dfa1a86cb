"""The public API of models.py does not move: every public callable of every class - inherited ones included, so a method that a
subclass no longer overrides must still resolve with the same signature and defaults - against the list recorded in
tests/golden/signatures.json (tests/golden/make_golden_signatures.py).  A new class is not an API change; a class, a method or a
default that the list holds and the module no longer gives is.  No GPU."""
import inspect
import json
import os

from poi_amd import models as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "signatures.json")


def public_signatures(names=None):
    """[[class, method, str(inspect.signature)]] of the public callables (and __init__) of the classes models.py defines - all of
    them, or the named ones - sorted by class and method."""
    if names is None:
        names = [n for n, c in vars(M).items() if inspect.isclass(c) and c.__module__ == M.__name__]
    rows = []
    for cname in sorted(names):
        cls = getattr(M, cname)
        for name in sorted(dir(cls)):
            attr = getattr(cls, name)
            if (name == "__init__" or not name.startswith("_")) and callable(attr):
                rows.append([cname, name, str(inspect.signature(attr))])
    return rows


def test_public_signatures_are_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    classes = sorted({row[0] for row in want})
    missing = [c for c in classes if not inspect.isclass(getattr(M, c, None))]
    assert not missing, "classes that left models.py: %s" % missing
    got = public_signatures(classes)
    assert len(want) > 300                                                      # the list is the whole module's, not a stub
    moved = [(w, g) for w, g in zip(want, got) if w != g]
    assert got == want, "first difference (recorded, current): %s" % (moved[0] if moved else "a method was added or removed")
