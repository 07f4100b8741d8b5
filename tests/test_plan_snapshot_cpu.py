"""``routes.plan`` and seeded construction against tests/golden/plan_snapshot.json.gz, recorded before ``detector.py`` got one pillar trunk and the fusion families
their own plan wording (tests/golden/make_plan_snapshot.py, which also states what the snapshot holds).  Everything is compared with ``==``: whole plans, ``fallbacks``
as an ordered list, ``state_dict`` keys in order with shapes and the SHA-256 of every seeded tensor.  A difference means the refactor changed a route decision, a
printed string, the order in which a model registers its submodules or the random numbers a parameter receives -- the snapshot is never regenerated to make it pass."""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location("make_plan_snapshot", os.path.join(os.path.dirname(__file__), "golden", "make_plan_snapshot.py"))
snap = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(snap)

SHIPPED = snap.shipped()


@pytest.fixture(scope="module")
def recorded():
    return snap.load()


def _sets():
    from test_routes_cpu import MUTANTS
    sets = [("config:" + n, h, False) for n, h in SHIPPED.items()] + [("mutant:" + n, h, False) for n, h in MUTANTS.items()]
    return sets + [("fallback:" + n, h, n.endswith("@window")) for n, h in snap.fallback_mutants().items()]


SETS = _sets()


def test_the_snapshot_holds_exactly_these_sets(recorded):
    assert list(recorded["plans"]) == [n for n, _, _ in SETS]
    assert list(recorded["state"]) == list(SHIPPED)


@pytest.mark.parametrize("name", [n for n, _, _ in SETS])
def test_plan_is_what_it_was(recorded, name):
    h, window = next((h, w) for n, h, w in SETS if n == name)
    got = snap._plans(h, window)
    want = recorded["plans"][name]
    assert list(got) == list(want)
    for t in got:
        assert got[t]["fallbacks"] == want[t]["fallbacks"], (name, t)
        assert got[t] == want[t], (name, t, {k: (got[t]["layers"].get(k), want[t]["layers"].get(k)) for k in set(got[t]["layers"]) | set(want[t]["layers"])
                                              if got[t]["layers"].get(k) != want[t]["layers"].get(k)})
        assert list(got[t]["layers"]) == list(want[t]["layers"]), (name, t)


@pytest.mark.parametrize("name", list(SHIPPED))
def test_seeded_state_dict_is_what_it_was(recorded, name):
    got, want = snap._state(SHIPPED[name]), recorded["state"][name]
    assert [r[:2] for r in got] == [r[:2] for r in want]          # keys in order, with shapes
    assert got == want                                             # and every tensor's bytes
