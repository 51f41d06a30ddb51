"""tests/step_pins.py itself, on every committed step fixture and every configuration in it, without a device: the
reference's own float64 and float32 runs pass `check`; a moved term, a moved table element and a NaN fail it and are all
named in the one message; a shrunk sensitivity figure trips the assert; the two tolerance forms and the table that assigns
them to the families are what the module's docstring says."""
import copy

import numpy as np
import pytest

import directau_fixture
import ssl4rec_fixture
import step_pins as sp

RECORDS = [sp.record(f, g, c) for f in ("ncl", "mhcn", "sept", "buir", "gcl", "lightgcn") for g in [sp.load(f)]
           for c in sp.configs(f, g)]
RECORDS += [cf.record() for cf in ssl4rec_fixture.load()[1]] + [cf.record() for cf in directau_fixture.load()[2]]
IDS = [f"{r.family}-{r.tag}".replace(" ", "") for r in RECORDS]
each_record = pytest.mark.parametrize("rec", RECORDS, ids=IDS)


def test_every_family_and_configuration_is_covered():
    assert {r.family for r in RECORDS} == set(sp.TABLE_FORM) == set(sp.TERM_FORM)
    assert len(RECORDS) == 3 + 2 + 2 + 2 + 1 + 4 + 3 + 3 and len(set(IDS)) == len(IDS)


@each_record
def test_the_references_own_runs_pass(rec):
    sp.check(rec, rec.f64, rec.tables)
    sp.check(rec, rec.f32, rec.tables)           # the writers assert |f32 - f64| <= REL x |f64|: inside either term form


@each_record
def test_injected_failures_are_all_named_in_one_message(rec):
    first, last, j = list(rec.tables)[0], list(rec.tables)[-1], len(rec.terms) - 1
    step = int(np.argmax(rec.tol[:, j]))
    terms, moved, nan = rec.f64.copy(), copy.deepcopy(rec.tables), copy.deepcopy(rec.tables)
    terms[step, j] += 2 * rec.tol[step, j]
    moved[first].flat[moved[first].size // 2] += 2 * rec.atol[first]
    nan[last].flat[0] = np.nan
    said = [f"{rec.terms[j]}: got", f"{first}: max |final - f64|", f"{last}: not finite"]
    assert rec.tol[step, j] > 0 and first != last
    for got_terms, got_tables, mine, want in ((terms, rec.tables, [], said[:1]), (rec.f64, moved, [], said[1:2]),
                                              (rec.f64, nan, [], said[2:]),
                                              (terms, dict(moved, **{last: nan[last]}), ["mine: kept"], said + ["mine: kept"])):
        with pytest.raises(AssertionError) as e:
            sp.check(rec, got_terms, got_tables, failures=mine)
        assert all(w in str(e.value) for w in want), (want, str(e.value))
    moved[first] = rec.tables[first] + 0.5 * rec.atol[first]          # inside the tolerances: passes
    sp.check(rec, rec.f64 + 0.5 * rec.tol, moved)


def _weaker(rec, attr, name, value):
    weak = copy.copy(rec)
    setattr(weak, attr, dict(getattr(rec, attr), **{name: value}))
    return weak


@each_record
def test_a_shrunk_sensitivity_figure_trips_the_assert(rec):
    rec.assert_sensitivity()
    assert rec.moved or (rec.dropped and rec.factor)          # every family asserts one of the two rules
    k, weak = list(rec.tables)[0], []
    if rec.dropped and rec.factor:                            # a term that moves the table by no more than the tolerance
        term = [t for t in rec.dropped[k] if k not in rec.unreached.get(t, ())][0]
        weak.append(_weaker(rec, "dropped", k, dict(rec.dropped[k], **{term: rec.atol[k]})))
    if rec.moved:                                             # a table that moved by 50 x slack
        weak.append(_weaker(rec, "moved", k, (rec.tables[k] - 50 * rec.moved[k][1], rec.moved[k][1])))
    for term, names in rec.unreached.items():                 # MHCN: no term reaches these; exactly 0.0 and nothing else
        assert all(rec.dropped[name][term] == 0.0 for name in names)
        weak += [_weaker(rec, "dropped", name, dict(rec.dropped[name], **{term: 1e-30})) for name in names]
    for w in weak:
        with pytest.raises(AssertionError):
            w.assert_sensitivity()
        with pytest.raises(AssertionError):
            sp.check(w, rec.f64, rec.tables)


def test_the_two_tolerance_forms():
    assert sp.atol_floor_1(0.0) == 1e-7 and sp.atol_floor_4(0.0) == 4e-7
    assert sp.atol_floor_1(1e-6) == sp.atol_floor_4(1e-6) == 4 * 1e-6
    assert (sp.REL, sp.F32, sp.FLOOR, sp.DROPPED, sp.DROPPED_CPU, sp.MOVED) == (1e-5, 4, 1e-7, 50, 10, 100)
    f64, f32 = np.array([2.0, -3.0, 0.0]), np.array([2.0 + 1e-4, -3.0, 0.0])
    assert sp.term_tol(f64).tolist() == [2e-5, 3.0000000000000004e-05, 0.0]
    assert sp.term_tol(f64, f32).tolist() == [4 * abs(f32[0] - 2.0), 3.0000000000000004e-05, 0.0]
    assert sp.difference_tol(np.array([2.0]), np.array([-3.0])).tolist() == [5e-5]
    a = 2.0 ** -23                                            # products with it are exact: the rules are strict
    assert sp.sees_dropped(51 * a, a) and not sp.sees_dropped(50 * a, a) and sp.sees_dropped(11 * a, a, factor=sp.DROPPED_CPU)
    assert sp.sees_dropped(0.0, a, unreached=True) and not sp.sees_dropped(1e-3, a, unreached=True)
    assert sp.has_moved(101 * a, a) and not sp.has_moved(100 * a, a)


def test_which_family_uses_which_form():
    floor_1 = {"ncl", "mhcn", "sept", "buir"}                       # max(4 x slack, 1e-7); the prepared-model tests read these
    floor_4 = {"gcl", "lightgcn", "ssl4rec", "directau"}            # 4 x max(slack, 1e-7)
    assert {f for f, form in sp.TABLE_FORM.items() if form is sp.atol_floor_1} == floor_1
    assert {f for f, form in sp.TABLE_FORM.items() if form is sp.atol_floor_4} == floor_4
    assert {f for f, form in sp.TERM_FORM.items() if form == "f32"} == floor_1
    assert {f for f, form in sp.TERM_FORM.items() if form == "rtol"} == floor_4
    for rec in RECORDS:
        for k, slack in rec.slack.items():
            assert rec.atol[k] == (max(slack * 4, 1e-7) if rec.family in floor_1 else max(slack, 1e-7) * 4)
