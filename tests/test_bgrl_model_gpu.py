"""BGRLModel on the device (every layer through the fused gcr_gin_* kernels, FusedAdam) against the reference's own
trajectories (tests/golden/bgrl_steps.npz, written from bgrl_g2l.py by scripts/gen_golden_bgrl_steps.py) under
tests/step_pins.py's rules, `predict` against the stored float64 scores, the state dict under the reference's names, the
`prepare` cache and one end-to-end `train()`."""
import numpy as np
import pytest
import torch

import gin_rules as gr
import step_pins as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return gr.load()


@pytest.mark.parametrize("case", gr.STEP_CASES)
def test_train_steps_follow_the_reference_trajectory(golden, case):
    """The recorded masks replayed; loss: `term_tol` with the float32 run; every final parameter and BatchNorm buffer of the
    online encoder, the predictor and the target encoder: `atol_floor_1`; `sees_dropped` and `has_moved` first.  Then
    `predict` in eval mode against the stored float64 scores, held like a final table (gin_rules.check_scores)."""
    cfg = gr.step_config(golden, case)
    model, losses = gr.run_steps(golden, case, "cuda", torch.float32)
    from recommendation_amd import functional as Fn
    assert Fn.gin_supported(cfg["hidden_dim"], cfg["hidden_dim"]) and all(c.fused for c in model.encoder.online_encoder.layers)
    assert type(model.optimizer).__name__ == "FusedAdam"
    gr.check_steps(golden, case, losses, gr.finals_of(model, cfg))
    got = np.stack([model.predict(int(u)) for u in golden[f"{case}/score_users"]])
    assert not model.encoder.training
    gr.check_scores(golden, case, got)


def test_the_layers_run_the_fused_node(golden):
    from recommendation_amd.bgrl import BGRLModel
    model = BGRLModel(dict(hidden_dim=64), gr.step_triples(golden, "A"), [], seed=3)
    model.encoder.train()
    z, _ = model.encoder.online_encoder(model.x, model.edge_index)
    assert not gr.no_fused_node_below(z), "the encoder must run gcr_gin_*"
    for conv in model.encoder.online_encoder.layers:
        conv.fused = False
    z2, _ = model.encoder.online_encoder(model.x, model.edge_index)
    assert gr.no_fused_node_below(z2)


def test_reference_named_state_round_trips_on_the_device(golden):
    from recommendation_amd.bgrl import BGRLModel
    train = gr.step_triples(golden, "A")
    a = BGRLModel({}, train, [], seed=1)
    a.train_step()
    state = {k: v.detach().cpu().clone() for k, v in a.encoder.state_dict().items()}
    assert {"online_encoder.layers.0.nn.0.weight", "online_encoder.batch_norm.norm.weight", "online_encoder.projection_head.0.weight",
            "predictor.2.weight", "target_encoder.layers.1.nn.2.bias"} <= set(state)
    b = BGRLModel({}, train, [], x=a.x, seed=2)
    b.load_reference_state({k: v for k, v in state.items() if not k.endswith(".eps")})       # with or without PyG's eps buffers
    for k, v in b.encoder.state_dict().items():
        assert v.is_cuda and torch.equal(v.cpu(), state[k]), k
    user = train[0][0]
    assert np.array_equal(a.predict(user), b.predict(user))


def test_prepare_obeys_the_cache_contract():
    from prepare_cache import check_prepare_cache
    from recommendation_amd import functional as Fn
    from recommendation_amd.bgrl import GConv
    conv = GConv(32, 32, 2, 0.2, torch.nn.ReLU).cuda()
    check_prepare_cache(lambda e: conv.prepare(e, 50), lambda e: Fn.gin_sum_graph(e, 50, "cuda"), 50, device="cuda")


def test_train_returns_finite_metrics_at_the_four_cutoffs():
    from recommendation_amd.bgrl import BGRLModel
    train, test, _ = sp.planted_group_lists(np.random.default_rng(0))
    model = BGRLModel({}, train, test, seed=0)
    assert model.topN == [10, 20, 30, 50] and model.maxEpoch == 1
    metrics = model.train()
    assert set(metrics) == {"Hit Ratio", "Precision", "Recall", "NDCG"} and all(np.isfinite(v) for v in metrics.values())
    # the draws are functions of the seed: the same seed gives the same model, another seed another
    again = BGRLModel({}, train, test, seed=0)
    again.train_step()
    other = BGRLModel({}, train, test, seed=1)
    other.train_step()
    w = lambda m: m.encoder.online_encoder.layers[0].nn[0].weight                    # noqa: E731
    assert torch.equal(w(model), w(again)) and not torch.equal(w(model), w(other))
    performance = model.fast_evaluation(0)
    assert set(performance) == set(metrics) and model.bestPerformance[0] == 1
