"""The workspace size queries of the loss, dense and BPR units (csrc/gcr_{buir,directau,tri,mim,bt,dense,bpr}.hip: one layout
function per unit on csrc/gcr_host.h's WsCarve, shared by the entry points and the query) against
tests/golden/launch_workspace.json, recorded by scripts/gen_launch_workspace_golden.py from the commit before the layouts
moved onto the carver: the sizes callers see are what they were, for every supported width, for an unsupported one, for empty
problems, at and past the batch bound, and for every shape the GPU tests of these units build.  The queries are host-only: no
device is touched."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("gen_launch_workspace_golden",
                                               os.path.join(ROOT, "scripts", "gen_launch_workspace_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

ALL_QUERIES = set(gen.QUERIES) | {"gcr_gram_tn_workspace_bytes", "gcr_tri_workspace_bytes"}


@pytest.fixture(scope="module")
def lib():
    from recommendation_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    with open(gen.GOLDEN) as f:
        return json.load(f)


def align256(x):
    return (x + 255) & ~255


def test_sizes_are_the_recorded_ones(lib, golden):
    """The two sorts' sizes contain rocPRIM's own temporary size, which rocPRIM derives from the device it sees: the file was
    recorded with none visible and is compared where none is visible (the build host).  With a device they are held to the
    part that is this library's: gcr_sort_index's two 256-byte aligned arrays of n four-byte words ahead of rocPRIM's
    storage (what gcr_sort_index itself carves), and 0 for an empty problem.  Every other query is a pure function of its
    arguments and is compared everywhere."""
    import torch
    assert set(golden) == ALL_QUERIES and set(gen.ROCPRIM_BACKED) < ALL_QUERIES
    device = torch.cuda.is_available()
    for name, rows in golden.items():
        fn = getattr(lib, name)
        for *args, want in rows:
            if device and name in gen.ROCPRIM_BACKED:
                own = 2 * align256(4 * args[0]) if name == "gcr_sort_index_workspace_bytes" else 0
                assert fn(*args) >= own and (args[0] > 0 or fn(*args) == 0), (name, args)
                assert want >= own
            else:
                assert fn(*args) == want, (name, args)
        # nothing is trivially equal: every query is non-zero somewhere, and all but the payload sort's (rocPRIM's own
        # temporary size, one value at every n recorded) vary with the shape
        assert any(r[-1] > 0 for r in rows), name
        assert len({r[-1] for r in rows}) > 3 or name == "gcr_sort_pairs_u64_workspace_bytes", name


def test_recorded_shapes_are_the_generators(golden):
    """A shape added to a GPU case table has to be recorded too (rerun the generator on a build whose sizes are trusted)."""
    cases = gen.cases()
    assert set(cases) == ALL_QUERIES
    for name, shapes in cases.items():
        assert [tuple(r[:-1]) for r in golden[name]] == shapes, name
    have = {name: {tuple(r[:-1]) for r in rows} for name, rows in golden.items()}
    for name, shapes in gen.body_shapes().items():
        assert shapes and shapes <= have[name], name
    # a few of the body shapes by name, so that an emptied table does not pass
    assert {(65, 512), (257, 48), (0, 64)} <= have["gcr_buir_workspace_bytes"]
    assert {(300, 512), (77, 48), (127, 32)} <= have["gcr_directau_workspace_bytes"]
    assert {(300001, 32), (70001, 256), (777, 256), (513, 64)} <= have["gcr_bt_workspace_bytes"]
    assert {(513, 48), (513, 1024)} <= have["gcr_col_stats_workspace_bytes"]
    assert {(10940, 32, 5), (1000, 64, 32), (257, 128, 32), (33, 32, 32)} <= have["gcr_tri_workspace_bytes"]
    assert {(263000, 32), (4353, 256), (20011, 32), (775, 32)} <= have["gcr_mim_workspace_bytes"]
    assert {(775, 32, 32)} <= have["gcr_gram_tn_workspace_bytes"]
    assert {(65539,), (32773 * 1,), (257 * 3,)} <= have["gcr_sort_pairs_u64_workspace_bytes"]


def test_every_width_every_row_count_and_the_bounds_are_there(golden):
    for name, (arity, ladder, supported, unsupported, bounded) in gen.QUERIES.items():
        rows = golden[name]
        assert {r[0] for r in rows} >= set(gen.ROWS), name
        if arity == 1:
            assert {r[0] for r in rows} >= set(gen.BATCH_BOUND), name
            continue
        assert {r[1] for r in rows if r[0] in gen.FEW_ROWS} >= set(supported), name
        for n in gen.ROWS + (gen.BATCH_BOUND if bounded else ()):
            assert {r[1] for r in rows if r[0] == n} >= set(ladder) | {unsupported}, (name, n)
        # the unsupported width and the empty problem return 0, as they did
        assert all(r[2] == 0 for r in rows if r[1] == unsupported or r[0] == 0), name
        assert all(r[2] > 0 for r in rows if 2 <= r[0] < gen.BATCH_BOUND[1] and r[1] in supported), name
    # gcr_buir_workspace_bytes refuses the batch its entry points refuse
    assert all(r[2] == 0 for r in golden["gcr_buir_workspace_bytes"] if r[0] == gen.BATCH_BOUND[1])
    assert all(r[2] > 0 for r in golden["gcr_buir_workspace_bytes"] if r[0] == gen.BATCH_BOUND[0] and r[1] != 40)
    gram = golden["gcr_gram_tn_workspace_bytes"]
    assert all((r[3] == 0) == (r[0] == 0 or gen.GRAM_UNSUPPORTED in r[1:3]) for r in gram)
    assert {(r[1], r[2]) for r in gram if r[3]} == {(dx, dg) for dx in gen.GRAM_DIMS for dg in gen.GRAM_DIMS}
    tri = golden["gcr_tri_workspace_bytes"]
    assert all(r[3] == 0 for r in tri if r[0] == 0 or r[1] == gen.TRI_UNSUPPORTED[0] or r[2] == gen.TRI_UNSUPPORTED[1])
    assert {(r[1], r[2]) for r in tri if r[3]} >= {(d, k) for d in gen.TRI_WIDTHS for k in gen.TRI_KS}
