"""NCLModel's training step pinned to ncl.py's own loop body (ncl.py:311-329) run in float64: tests/golden/ncl_steps.npz,
written by scripts/gen_golden_ncl_steps.py.  Six batches from the fixture's initial tables, three configurations (the
context layer interior, the last one by the `>= len(emb_list)` branch, the last one by index at d = 128), four paths:

  * autograd      train_step(fused=False) with FusedAdam;
  * fused         train_step(fused=True): FusedNCLStep run eagerly;
  * graph         NCLModel(graph_capture=True) with FusedAdam(capturable=True), replayed from a hipGraph;
  * resume_*      three steps, a torch.save / torch.load checkpoint of model and optimizer, a fresh model and optimizer
                  that finish the steps: capturable -> capturable, capturable -> not, not -> capturable.

The e_step (faiss k-means in the reference) is the one stand-in, on both sides: fixed centroids from the fixture, each
row assigned to its nearest centroid of the current encoder output (the real assignment kernel here).  The generator has
checked that no row the prototype contrast reads comes near a tie.

The rule is tests/step_pins.py's (family "ncl"): terms against the reference's float64 and float32 runs, final tables
within `atol_floor_1` of the reference's own f32 slack, and that tolerance at most 1/50 of what dropping the structure
contrast, the prototype contrast or the l2 term would move the table."""
import io

import numpy as np
import pytest
import torch

import step_pins as sp
from step_pins import NCL_TERMS as TERMS  # noqa: F401  (tests/test_prepared_models_gpu.py reads it from here)

pytestmark = pytest.mark.gpu

TABLES = ("user_emb", "item_emb")
PATHS = ("autograd", "fused", "graph", "resume_cap_cap", "resume_cap_eager", "resume_eager_cap")


@pytest.fixture(scope="module")
def steps():
    return sp.load("ncl")


def _conf(g, c):
    return {"model": {"name": "NCL", "type": "graph"}, "embedding.size": int(g[f"c{c}/d"]),
            "batch.size": int(g["batch_size"]), "learning.rate": float(g["hp/learning.rate"]),
            "reg.lambda": float(g["hp/reg.lambda"]), "max.epoch": 1, "item.ranking.topN": [10],
            "NCL": {"n_layers": int(g[f"c{c}/n_layers"]), "tau": float(g["hp/NCL.tau"]),
                    "ssl_reg": float(g["hp/NCL.ssl_reg"]), "proto_reg": float(g["hp/NCL.proto_reg"]),
                    "alpha": float(g["hp/NCL.alpha"]), "num_clusters": int(g[f"c{c}/user_centroids"].shape[0]),
                    "hyper_layers": int(g[f"c{c}/hyper_layers"])}}


@pytest.fixture
def fixed_e_step(monkeypatch, steps):
    """Returns a function c -> None that makes NCLModel.e_step use configuration c's fixed centroids: `run_kmeans`
    hands back a preallocated device copy and, when asked for assignments, the real assignment kernel's.  No host
    read-back, so it is capturable and safe on the e_step's side streams."""
    from recommendation_amd import ncl as ncl_mod
    from recommendation_amd.kmeans import assign_to_centroids

    def use(c):
        g = steps
        cents = {}
        for side in ("user", "item"):
            cent = torch.from_numpy(g[f"c{c}/{side}_centroids"]).cuda()
            n = len(g[f"{side}_ids"])
            assert n not in cents
            cents[n] = cent

        def run_kmeans(x, k, niter=None, seed=None, assign_points=True):
            cent = cents[x.shape[0]]
            return cent, (assign_to_centroids(x, cent) if assign_points else None)

        monkeypatch.setattr(ncl_mod, "run_kmeans", run_kmeans)
    return use


def _model(g, c, **kw):
    from recommendation_amd.ncl import NCLModel
    train = sp.triples(g)
    m = NCLModel(_conf(g, c), train, train[:20], device="cuda", **kw)
    sp.assert_dense_id_order(m, g)                                  # sorted raw ids, ncl.py:60-61
    d = int(g[f"c{c}/d"])
    with torch.no_grad():
        for k in TABLES:
            m.model.embedding_dict[k].copy_(torch.from_numpy(g[f"init_d{d}/{k}"]))
    return m


def _optimizer(g, m, capturable):
    from recommendation_amd.optim import FusedAdam
    return FusedAdam(m.model.parameters(), lr=float(g["hp/learning.rate"]), capturable=capturable)


def _batches(g):
    return [sp.batch(g, n, ("users", "pos", "neg")) for n in range(int(g["steps"]))]


def _run(m, opt, batches, fused):
    """train_step over the batches; the four losses of every step, copied out (a replayed graph overwrites its outputs)."""
    out = []
    for batch in batches:
        res = m.train_step(batch, opt, check_negatives=False, fused=fused)
        out.append(torch.stack([t.detach().reshape(()) for t in res]).clone())
    return out


def _graph_ran(m, opt, n_steps):
    assert m._fused is not None and m._fused._cuda_graph is not None         # the step really replayed from a graph
    for p in m.model.parameters():
        assert int(opt.state[p]["step_dev"]) == n_steps


def _resume(g, c, src_cap, dst_cap, batches):
    half = len(batches) // 2
    src = _model(g, c, graph_capture=src_cap)
    o_src = _optimizer(g, src, src_cap)
    losses = _run(src, o_src, batches[:half], fused=True)
    buf = io.BytesIO()
    torch.save({"model": src.model.state_dict(), "opt": o_src.state_dict()}, buf)
    buf.seek(0)
    ckpt = torch.load(buf, weights_only=True)
    del src, o_src
    dst = _model(g, c, graph_capture=dst_cap)
    dst.model.load_state_dict(ckpt["model"])
    o_dst = _optimizer(g, dst, dst_cap)
    o_dst.load_state_dict(ckpt["opt"])
    for p in dst.model.parameters():
        st = o_dst.state[p]
        assert st["step"] == half
        if dst_cap:
            assert st["step_dev"].dtype == torch.int64 and int(st["step_dev"]) == half
    losses += _run(dst, o_dst, batches[half:], fused=True)
    if dst_cap:
        _graph_ran(dst, o_dst, len(batches))
    return dst, losses


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("c", [0, 1, 2])
def test_ncl_trajectory_matches_reference_float64(steps, fixed_e_step, c, path):
    from recommendation_amd.ncl_step import FusedNCLStep
    g = steps
    fixed_e_step(c)
    batches = _batches(g)
    if path == "autograd":
        m = _model(g, c, fused_step=False)
        losses = _run(m, _optimizer(g, m, False), batches, fused=False)
    elif path == "fused":
        m = _model(g, c)
        assert FusedNCLStep.supported(m)
        losses = _run(m, _optimizer(g, m, False), batches, fused=True)
    elif path == "graph":
        m = _model(g, c, graph_capture=True)
        opt = _optimizer(g, m, True)
        losses = _run(m, opt, batches, fused=True)
        _graph_ran(m, opt, len(batches))
    else:
        src_cap, dst_cap = {"resume_cap_cap": (True, True), "resume_cap_eager": (True, False),
                            "resume_eager_cap": (False, True)}[path]
        m, losses = _resume(g, c, src_cap, dst_cap, batches)
    got = torch.stack(losses).cpu().numpy().astype(np.float64)            # [steps, 4]
    final = {k: m.model.embedding_dict[k].detach().cpu().numpy().astype(np.float64) for k in TABLES}

    sp.check(sp.record("ncl", g, c, path), got, final)
