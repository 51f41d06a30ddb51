"""recommendation_amd/spmm_launch.py against the parameter NAMES of include/gcr.h: every launch function is called with a
distinct value per argument, through `_lib.call_on` over a stand-in handle that records what it is given, and each value
must arrive at the position of the header's parameter of that name.  tests/test_abi_cpu.py holds the types; two adjacent
`float*` or `int64_t` arguments swapped pass there and fail here.  No device and no built library needed."""
import inspect
import types
from ctypes import c_float, c_void_p

import pytest
import torch

from gcr_header import header_prototypes
from recommendation_amd import _lib
from recommendation_amd import spmm_launch as L

LAUNCHES = {"gcr_spmm_csr_acc2_f32": L.csr_acc2, "gcr_spmm_csr_dual_f32": L.csr_dual, "gcr_spmm_csr_dual_acc_f32": L.csr_dual_acc,
            "gcr_spmm_rows_f32": L.rows, "gcr_spmm_hub_parts_f32": L.hub_parts, "gcr_spmm_hub_reduce_f32": L.hub_reduce,
            "gcr_spmm_windowed_f32": L.windowed}
# A keyword goes to the header's parameter of the same name.  Where a positional argument's fields go: field -> parameter
CSR = {"rowptr": "rowptr", "col": "col", "val": "val"}
PLAN = {"desc": "desc", "n_parts": "n_parts", "long_row": "long_row", "long_slot0": "long_slot0", "n_long": "n_long_rows"}
FIELDS = {"graph": {**CSR, "n_rows": "n_rows", "n_cols": "n_cols"}, "plan": PLAN,
          "hub_graph": {f: "hub_" + p for f, p in CSR.items()},              # the companion's own n_rows / n_cols go nowhere
          "hub_plan": {f: "hub_" + p for f, p in PLAN.items()},
          "hub": {"hub_row": "hub_row", "n_hub": "n_hub", "n_windows": "n_windows"}}
# what `functional.spmm_into` passes for an argument its caller omits
DEFAULTS = {"y": None, "acc_in": None, "acc_in2": None, "acc_out": None, "y_norm": None, "keep_bits": None, "inv_norm_out": None,
            "col_active_bits": None, "val_scale": 1.0, "acc_scale": 1.0, "acc_in2_scale": 1.0, "flags": 0}
STREAM = 0x5EED0
PROTOS = header_prototypes()


@pytest.fixture
def recorded():
    """(call, seen): a `call` over a handle with the seven exports as functions that append (name, args) to `seen`."""
    seen = []
    handle = types.SimpleNamespace(**{name: (lambda *args, name=name: seen.append((name, args)) or 0) for name in LAUNCHES})
    call = _lib.call_on(handle)
    assert all(call.has(name) for name in LAUNCHES) and not call.has("gcr_version")
    return call, seen


def _arguments(name, only_required=False):
    """(positional objects, keywords, {header parameter: the value that must arrive there}) for one launch function: a
    one-element CPU tensor of its own per pointer, a number of its own per scalar."""
    _, kinds, params = PROTOS[name]
    fresh = iter(range(3, 1000, 2))

    def sentinel(param):
        kind = kinds[params.index(param)]
        if kind is c_void_p:
            t = torch.zeros(1)
            return t, t.data_ptr()
        v = next(fresh) + 0.5 if kind is c_float else next(fresh)
        return v, v

    positional, keywords, want = [], {}, {}
    for arg, p in inspect.signature(LAUNCHES[name]).parameters.items():
        if p.kind is p.POSITIONAL_OR_KEYWORD:
            obj = types.SimpleNamespace(n_rows=-1, n_cols=-2)
            for field, param in FIELDS[arg].items():
                value, want[param] = sentinel(param)
                setattr(obj, field, value)
            positional.append(obj)
        elif arg not in ("on", "call") and not (only_required and p.default is not p.empty):
            keywords[arg], want[arg] = sentinel(arg)
    return positional, keywords, want


def _launch(name, recorded, **kw):
    call, seen = recorded
    positional, keywords, want = _arguments(name, **kw)
    assert LAUNCHES[name](*positional, **keywords, on=c_void_p(STREAM), call=call) is None
    (got_name, args), = seen
    assert got_name == name and len(args) == len(PROTOS[name][2])
    return dict(zip(PROTOS[name][2], args)), want, keywords


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_every_argument_arrives_at_the_headers_parameter_of_its_name(name, recorded):
    got, want, _ = _launch(name, recorded)
    params = PROTOS[name][2]
    assert sorted([*want, "stream"]) == sorted(params),"an argument the header does not name, or a parameter nothing fills"
    assert len(set(want.values())) == len(want), "two arguments share a value"
    for param in params[:-1]:
        assert got[param] == want[param], f"{name}: `{param}` received another argument's value"
    assert params[-1] == "stream" and got["stream"].value == STREAM


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_an_omitted_argument_is_what_spmm_into_passes(name, recorded):
    got, want, given = _launch(name, recorded, only_required=True)
    omitted = [arg for arg, p in inspect.signature(LAUNCHES[name]).parameters.items()
               if p.kind is p.KEYWORD_ONLY and arg not in given and arg not in ("on", "call")]
    assert omitted or name == "gcr_spmm_hub_parts_f32"
    for arg in omitted:
        assert got[arg] == DEFAULTS[arg] and type(got[arg]) is type(DEFAULTS[arg]), f"{name}: default of `{arg}`"
    for param, value in want.items():
        assert got[param] == value, f"{name}: `{param}`"


def test_windowed_takes_the_companion_pair_first_and_the_main_pair_second(recorded):
    call, seen = recorded
    (hub_graph, hub_plan, graph, plan, hub), keywords, _ = _arguments("gcr_spmm_windowed_f32")
    graph.n_rows, graph.n_cols, hub_graph.n_rows, hub_graph.n_cols = 11, 12, 13, 14
    L.windowed(hub_graph, hub_plan, graph, plan, hub, **keywords, on=c_void_p(STREAM), call=call)
    got = dict(zip(PROTOS["gcr_spmm_windowed_f32"][2], seen[0][1]))
    for prefix, csr, pl in (("hub_", hub_graph, hub_plan), ("", graph, plan)):
        assert [got[prefix + p] for p in ("desc", "n_parts", "long_row", "long_slot0", "n_long_rows", "rowptr", "col", "val")] == \
            [pl.desc.data_ptr(), pl.n_parts, pl.long_row.data_ptr(), pl.long_slot0.data_ptr(), pl.n_long,
             csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr()]
    assert (got["n_rows"], got["n_cols"]) == (11, 12), "the output's rows and the table's are the main graph's"
    assert got["hub_split"] == keywords["hub_split"].data_ptr() and got["partials"] == keywords["partials"].data_ptr()
